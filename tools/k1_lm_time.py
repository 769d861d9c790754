"""Scratch: K1's two-rate instantiation (bd_matrix_lm.hip) next to the lambda = mu one (bd_matrix.hip) -- sibling of tools/k1_time.py.  The HIP-event time
of the matrix build inside scorer calls (stats `ms_matrices`) and the whole call (`ms_total`) at the bench's matrix shape
(order 751, K = 8: 1320 matrices), on one context in one process: without death rates (K1), with mu = lambda (the two-rate
kernel on K1's own values) and with mu = 0.7 lambda."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cafexp_amd import capi, problem as P, synth
from cafexp_amd.gamma_rates import discrete_gamma

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10

pb, _ = synth.make_problem(n_families=2048)
probs, mult = discrete_gamma(8, 2.0)
lam = np.array([0.002])
pr = P.Params(lambdas=lam, prior=P.prior_uniform(pb.max_root_family_size), multipliers=mult, cat_probs=probs)
ctx = capi.Context(pb, max_categories=8)
ctx.set_profiling(True)
for label, mus in (("no death rates (K1)", None), ("mu = lambda (two-rate K1)", lam), ("mu = 0.7 lambda (two-rate K1)", 0.7 * lam),
                   ("no death rates (K1), again", None)):
    ctx.set_death_rates(mus)
    k1, total = [], []
    for i in range(reps + 2):
        v = ctx.score(pr, alpha=2.0)
        if i >= 2:
            st = ctx.stats()
            k1.append(st["ms_matrices"])
            total.append(st["ms_total"])
    print("order %d, K=8, %-30s matrices min %.4f median %.4f ms; call min %.3f median %.3f ms (%d matrices, -lnL %.6f)"
          % (pb.matrix_size, label + ":", min(k1), float(np.median(k1)), min(total), float(np.median(total)), st["n_matrices"], v), flush=True)
ctx.close()
