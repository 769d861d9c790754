#!/usr/bin/env python3
"""cafe_score_gain (the dense prune, gain_dense.hip) next to cafe_score_per_family_gain with the same rates tiled.

    python tools/gain_dense_time.py [--scaled] [OUT.json]     (on a machine with the GPU; --scaled: cafe_set_gain_scaling on)

One process.  The two lists DESIGN section 8 quotes for the gain entry: the distinct families of the mammals table (order 141,
7 repetitions) and 3000 families of the bench table (100 taxa, order 751, 3 repetitions), ONE rate set for the list, mu = lambda,
at nu = 0 and at nu = 0.3 lambda, root_absent 0.1, sum rule.  The two calls are alternated, host wall around each (both
synchronise); median, minimum and maximum of the repetitions after one warm-up pair, which also compares the values.  Then, in
calls of their own under cafe_set_profiling, the dense entry's split -- HIP-event ms of its build, product, GEMM and root
launches -- and the GEMM's rate over the flops it issues (whole 64 x 16 tiles, every column of the batch)."""
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


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


def alternated(name, pb, fam, lam, nu_over_lam, reps):
    pr = P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(pb.max_root_family_size))
    nu = nu_over_lam * lam
    tiled = [np.full(len(fam), x) for x in (lam, lam, nu)]
    ctx = capi.Context(pb)
    times = {"cafe_score_per_family_gain": [], "cafe_score_gain": []}
    try:
        ctx.set_root_rule("sum")
        if SCALED:
            ctx.set_gain_scaling(True)
        calls = {"cafe_score_per_family_gain": lambda: ctx.score_per_family_gain(pr, fam, *tiled, 0.1),
                 "cafe_score_gain": lambda: ctx.score_gain(pr, fam, [lam], [lam], [nu], 0.1)}
        a, b = calls["cafe_score_per_family_gain"](), calls["cafe_score_gain"]()
        both = np.isfinite(a) & np.isfinite(b)
        mismatched = int((np.isfinite(a) != np.isfinite(b)).sum())
        rel = float(np.max(np.abs(a[both] - b[both]) / np.abs(a[both])))
        for _ in range(reps):
            for what, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[what].append((time.perf_counter() - t0) * 1e3)
        ctx.set_profiling(True)
        split = []
        for _ in range(reps):
            calls["cafe_score_gain"]()
            ms, flops = ctx.gain_dense_profile()
            split.append(list(ms) + [flops])
        ctx.set_profiling(False)
    finally:
        ctx.close()
    rows = []
    for what, t in times.items():
        rows.append(dict(table=name, families=len(fam), branches=pb.n_nodes - 1, matrix_order=pb.matrix_size, nu_over_lambda=nu_over_lam, call=what,
                         repetitions=reps, median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)))
        print(json.dumps(rows[-1]), flush=True)
    med = np.median(np.array(split), axis=0)
    rows.append(dict(table=name, scaled=SCALED, nu_over_lambda=nu_over_lam, ratio_of_medians=rows[0]["median_ms"] / rows[1]["median_ms"], finite=int(both.sum()), finite_in_one_only=mismatched,
                     largest_relative_difference=rel, build_ms=med[0], product_ms=med[1], gemm_ms=med[2], root_ms=med[3], gemm_flops_issued=med[4],
                     gemm_tflops=med[4] / (med[2] * 1e-3) / 1e12 if med[2] > 0 else None))
    print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    species, ids, counts = P.read_family_table(read("mammal_gene_families.txt"))
    mammals = P.build_problem(P.parse_newick(read("mammals_tree.txt")), species, ids, counts)
    distinct = np.sort(np.unique(mammals.counts, axis=0, return_index=True)[1])
    bench, _ = synth.make_problem(n_taxa=100, n_families=3000, max_count=600)
    rows = []
    for ratio in (0.0, 0.3):
        rows += alternated("mammal_gene_families.txt, distinct families", mammals, distinct, 0.005, ratio, 7)
        rows += alternated("bench table (100 taxa, order 751)", bench, np.arange(bench.n_families), 0.002, ratio, 3)
    out = [a for a in sys.argv[1:] if a != "--scaled"]
    if out:
        with open(out[0], "w") as f:
            json.dump({"rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
