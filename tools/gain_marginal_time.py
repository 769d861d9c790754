#!/usr/bin/env python3
"""cafe_gain_marginal_dense (posterior sizes, intervals and expansion per branch on the dense prune) next to
cafe_gain_posterior_dense, its yardstick, at the same rates.

    python tools/gain_marginal_time.py [--scaled] [OUT.json]     (on a machine with the GPU; --scaled: cafe_set_gain_scaling on)

One process.  The two lists of DESIGN section 8: the distinct families of the mammals table (order 141, 7 repetitions) and 3000
families of the bench table (100 taxa, order 751, 3 repetitions), mu = lambda, nu = 0.3 lambda, root_absent 0.1, level 0.95.  The
two calls are alternated, host wall around each (both synchronise); median, minimum and maximum of the repetitions after one
warm-up pair, whose `mean` outputs are compared first.  Then the kernel split of both calls from their debug entries under
profiling, and the issued TFLOP/s of the split GEMM (its masked repeats counted) beside the transposed GEMM's of the same run; the
up GEMM's flops are those cafe_score_gain issues on the same list."""
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
KINDS = ("build", "product", "gemm", "root", "weights", "split_gemm", "interior_summary", "leaf_summary", "total")


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


def alternated(name, pb, fam, lam, reps):
    pr = P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(pb.max_root_family_size))
    rates = ([lam], [lam], [0.3 * lam], 0.1)
    times = {"cafe_gain_posterior_dense": [], "cafe_gain_marginal_dense": []}
    ctx = capi.Context(pb)
    try:
        if SCALED:
            ctx.set_gain_scaling(True)
        calls = {"cafe_gain_posterior_dense": lambda: ctx.gain_posterior_dense(pr, fam, *rates),
                 "cafe_gain_marginal_dense": lambda: ctx.gain_marginal_dense(pr, fam, *rates, 0.95)}
        a, b = calls["cafe_gain_posterior_dense"](), calls["cafe_gain_marginal_dense"]()
        assert np.array_equal(a["lnl"], b["lnl"], equal_nan=True)
        finite = np.isfinite(a["lnl"])
        rel = float(np.max(np.abs(a["mean"][finite] - b["mean"][finite]) / np.maximum(np.abs(a["mean"][finite]), 1e-290))) if finite.any() else 0.0
        for _ in range(reps):
            for what, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[what].append((time.perf_counter() - t0) * 1e3)
        ctx.set_profiling(True)
        ctx.set_root_rule("sum")
        ctx.score_gain(pr, fam, *rates)
        up_flops = ctx.gain_dense_profile()[1]
        yard, split = [], []
        for _ in range(reps):
            calls["cafe_gain_posterior_dense"]()
            ms, flops = ctx.gain_dense_posterior_profile()
            yard.append(list(ms) + [flops])
            calls["cafe_gain_marginal_dense"]()
            ms, flops = ctx.gain_marginal_profile()
            split.append(list(ms) + [flops])
        ctx.set_profiling(False)
    finally:
        ctx.close()
    rows = []
    for what, t in times.items():
        rows.append(dict(table=name, families=len(fam), finite=int(finite.sum()), branches=pb.n_nodes - 1, matrix_order=pb.matrix_size, call=what,
                         repetitions=reps, median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)))
        print(json.dumps(rows[-1]), flush=True)
    med, ymed = np.median(np.array(split), axis=0), np.median(np.array(yard), axis=0)
    row = dict(table=name, scaled=SCALED, ratio_to_the_yardstick=rows[1]["median_ms"] / rows[0]["median_ms"], largest_relative_difference_of_mean=rel)
    row.update({k + "_ms": float(v) for k, v in zip(KINDS, med)})
    row.update(yardstick_gemm_t_ms=float(ymed[5]), yardstick_interior_ms=float(ymed[6]), yardstick_leaf_ms=float(ymed[7]),
               split_gemm_tflops=(med[9] - up_flops) / (med[5] * 1e-3) / 1e12 if med[5] > 0 else None,
               gemm_t_tflops=(ymed[8] - up_flops) / (ymed[5] * 1e-3) / 1e12 if ymed[5] > 0 else None)
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
