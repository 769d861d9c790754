"""cafe_sample_histories beside cafe_marginal_reconstruct on one context of the bench table (50 000 families, 100 taxa,
N = 751): wall time of each call, base model and gamma K = 8, 100 draws, with and without the sizes array.  Every call is
timed REPS times and all times are kept (a call's first run pays for mapping its fresh workspace and output arrays); the
ratio is between the medians.  One process, one GPU; writes profiles/history_time.json (or the path given after the family
count)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from cafexp_amd import capi, problem as P, synth
from cafexp_amd.gamma_rates import discrete_gamma

DRAWS = 100
REPS = 3


def timed(fn):
    out, secs = None, []
    for _ in range(REPS):
        del out
        t = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t)
    return out, secs


def main():
    F = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "history_time.json")
    pb, _ = synth.make_problem(n_families=F)
    base = P.Params(lambdas=np.array([0.002]), prior=P.prior_uniform(pb.max_root_family_size))
    gamma = P.Params(lambdas=np.array([0.002]), prior=base.prior)
    gamma.cat_probs, gamma.multipliers = discrete_gamma(8, 2.0)
    ctx = capi.Context(pb, max_categories=8)
    ctx.score(base)
    lines = []
    for model, pr, alpha in (("base", base, 1.0), ("gamma_k8", gamma, 2.0)):
        marg, marginal_s = timed(lambda: ctx.marginal_reconstruct(pr, alpha=alpha))
        for sizes in (False, True):
            got, seconds = timed(lambda: ctx.sample_histories(pr, DRAWS, 1, alpha=alpha, sizes=sizes))
            rec = {"model": model, "families": pb.n_families, "unique_families": int(ctx.stats()["n_unique_families"]), "nodes": pb.n_nodes,
                   "matrix_order": pb.matrix_size, "draws": DRAWS, "sizes": sizes, "sample_histories_seconds": seconds,
                   "marginal_reconstruct_seconds": marginal_s, "ratio": float(np.median(seconds) / np.median(marginal_s)), "failed": int(got["failed"].sum()),
                   "marginal_failed": int(marg["failed"].sum())}
            del got
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    ctx.close()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": "AMD Instinct MI355X", "runs": lines}, f, indent=1)


if __name__ == "__main__":
    main()
