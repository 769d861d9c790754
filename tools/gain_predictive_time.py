#!/usr/bin/env python3
"""cafe_gain_leaf_predictive (the dense prune, its down pass and the fused leaf kernel) next to cafe_gain_posterior_dense on the
same lists.

    python tools/gain_predictive_time.py [--scaled] [OUT.json]     (on a machine with the GPU; --scaled: cafe_set_gain_scaling on)

One process.  The two lists of DESIGN section 8: the distinct families of the mammals table (order 141, 7 repetitions) and 3000
families of the bench table (100 taxa, order 751, 3 repetitions), mu = lambda, nu = 0.3 lambda, root_absent 0.1.  The two calls
are alternated, host wall around each (both synchronise); median, minimum and maximum of the repetitions after one warm-up pair.
Then the kernel split of the new call from cafe_debug_gain_predictive under profiling, and the issued TFLOP/s of the transposed
GEMM -- the yardstick: the same tile, in the same call, with a storing epilogue -- and of the fused kernel beside it.  The flops
of each come from differences of the three calls' counters: cafe_score_gain issues the up GEMM's, cafe_gain_posterior_dense adds
the transposed GEMM's, this call adds the fused kernel's."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cafexp_amd import capi, problem as P, synth  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
SCALED = "--scaled" in sys.argv[1:]
KINDS = ("build", "product", "gemm", "root", "weights", "gemm_t", "fused_leaf")


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


def alternated(name, pb, fam, lam, reps):
    pr = P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(pb.max_root_family_size))
    args = (pr, fam, [lam], [lam], [0.3 * lam], 0.1)
    ctx = capi.Context(pb)
    times = {"cafe_gain_posterior_dense": [], "cafe_gain_leaf_predictive": []}
    try:
        ctx.set_gain_scaling(SCALED)
        calls = {"cafe_gain_posterior_dense": lambda: ctx.gain_posterior_dense(*args), "cafe_gain_leaf_predictive": lambda: ctx.gain_leaf_predictive(*args)}
        finite = int(np.isfinite(calls["cafe_gain_posterior_dense"]()["lnl"]).sum())
        cells = calls["cafe_gain_leaf_predictive"]()["p_obs"]
        for _ in range(reps):
            for what, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[what].append((time.perf_counter() - t0) * 1e3)
        ctx.set_profiling(True)
        ctx.set_root_rule("sum")
        ctx.score_gain(*args)
        up_flops = ctx.gain_dense_profile()[1]
        calls["cafe_gain_posterior_dense"]()
        down_flops = ctx.gain_dense_posterior_profile()[1]
        split = []
        for _ in range(reps):
            calls["cafe_gain_leaf_predictive"]()
            ms, flops = ctx.gain_predictive_profile()
            split.append(list(ms) + [flops])
        ctx.set_profiling(False)
    finally:
        ctx.close()
    rows = []
    for what, t in times.items():
        rows.append(dict(table=name, families=len(fam), finite=finite, taxa=pb.n_taxa, matrix_order=pb.matrix_size, call=what, repetitions=reps,
                         median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)))
        print(json.dumps(rows[-1]), flush=True)
    med = np.median(np.array(split), axis=0)
    row = dict(table=name, scaled=SCALED, cells_with_a_distribution=int(np.isfinite(cells).sum()))
    row.update({k + "_ms": float(v) for k, v in zip(KINDS, med)})
    row.update(gemm_t_tflops=(down_flops - up_flops) / (med[5] * 1e-3) / 1e12 if med[5] > 0 else None,
               fused_leaf_tflops=(med[7] - down_flops) / (med[6] * 1e-3) / 1e12 if med[6] > 0 else None)
    rows.append(row)
    print(json.dumps(row), flush=True)
    return rows


def main():
    species, ids, counts = P.read_family_table(read("mammal_gene_families.txt"))
    mammals = P.build_problem(P.parse_newick(read("mammals_tree.txt")), species, ids, counts)
    distinct = np.sort(np.unique(mammals.counts, axis=0, return_index=True)[1])
    bench, _ = synth.make_problem(n_taxa=100, n_families=3000, max_count=600)
    rows = alternated("mammal_gene_families.txt, distinct families", mammals, distinct, 0.005, 7) + \
        alternated("bench table (100 taxa, order 751)", bench, np.arange(bench.n_families), 0.002, 3)
    out = [a for a in sys.argv[1:] if a != "--scaled"]
    if out:
        with open(out[0], "w") as f:
            json.dump({"rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
