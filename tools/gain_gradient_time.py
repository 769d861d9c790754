#!/usr/bin/env python3
"""cafe_gain_score_gradient (score vectors in lambda, mu, nu on the dense prune) next to cafe_gain_posterior_dense, its yardstick,
at the same rates.

    python tools/gain_gradient_time.py [OUT.json]     (on a machine with the GPU)

One process.  The two lists of DESIGN section 8: the distinct families of the mammals table (order 141, 7 repetitions) and 3000
families of the bench table (100 taxa, order 751, 3 repetitions), mu = lambda, nu = 0.3 lambda, root_absent 0.1.  The two calls are
alternated, host wall around each (both synchronise); median, minimum and maximum of the repetitions after one warm-up pair, whose
lnl are compared first.  Then the kernel split of both calls from their debug entries under profiling, the issued TFLOP/s of the
Toeplitz GEMM and of the second outside GEMM beside the transposed GEMM's of the same run (flops counted as the kernels issue them:
whole 64-row tiles, K tiles from the diagonal on for the Toeplitz GEMM), and the leaf filters' time."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cafexp_amd import capi, problem as P, synth  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
KINDS = ("build", "product", "gemm", "root", "weights", "gemm_t", "interior_score", "leaf_score", "outside2_gemm", "toeplitz_gemm", "leaf_filters", "total")


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


def alternated(name, pb, fam, lam, reps):
    pr = P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(pb.max_root_family_size))
    rates = ([lam], [lam], [0.3 * lam], 0.1)
    times = {"cafe_gain_posterior_dense": [], "cafe_gain_score_gradient": []}
    ctx = capi.Context(pb)
    try:
        calls = {"cafe_gain_posterior_dense": lambda: ctx.gain_posterior_dense(pr, fam, *rates),
                 "cafe_gain_score_gradient": lambda: ctx.gain_score_gradient(pr, fam, *rates)}
        a, b = calls["cafe_gain_posterior_dense"](), calls["cafe_gain_score_gradient"]()
        assert np.array_equal(a["lnl"], b["lnl"], equal_nan=True)
        finite = np.isfinite(a["lnl"])
        for _ in range(reps):
            for what, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[what].append((time.perf_counter() - t0) * 1e3)
        ctx.set_profiling(True)
        yard, grad = [], []
        for _ in range(reps):
            calls["cafe_gain_posterior_dense"]()
            ms, flops = ctx.gain_dense_posterior_profile()
            yard.append(list(ms) + [flops])
            calls["cafe_gain_score_gradient"]()
            ms, flops = ctx.gain_gradient_profile()
            grad.append(list(ms) + [flops])
        ctx.set_profiling(False)
    finally:
        ctx.close()
    rows = []
    for what, t in times.items():
        rows.append(dict(table=name, families=len(fam), finite=int(finite.sum()), branches=pb.n_nodes - 1, matrix_order=pb.matrix_size, call=what,
                         repetitions=reps, median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)))
        print(json.dumps(rows[-1]), flush=True)
    med, ymed = np.median(np.array(grad), axis=0), np.median(np.array(yard), axis=0)
    # what the gradient call issues on top of the yardstick's flops: per interior non-root node the Toeplitz triangle (whole 64-row
    # tiles, K tiles from the diagonal on) and the second outside GEMM, which is the rest
    n, cols = pb.max_family_size + 1, -(-len(fam) // 128) * 128
    n_int = int(np.sum((pb.leaf_taxon < 0) & (pb.parent >= 0)))
    tri = sum(2.0 * 64 * (-(-n // 16) * 16 - r0) * cols for r0 in range(0, n, 64))
    extra = med[12] - ymed[8]
    row = dict(table=name, ratio_to_the_yardstick=rows[1]["median_ms"] / rows[0]["median_ms"], interior_non_root_nodes=n_int,
               yardstick_flops=float(ymed[8]), gradient_flops=float(med[12]))
    row.update({k + "_ms": float(v) for k, v in zip(KINDS, med)})
    row.update(yardstick_gemm_t_ms=float(ymed[5]), yardstick_interior_ms=float(ymed[6]), yardstick_leaf_ms=float(ymed[7]),
               toeplitz_tflops=n_int * tri / (med[9] * 1e-3) / 1e12 if med[9] > 0 else None,
               outside2_tflops=(extra - n_int * tri) / (med[8] * 1e-3) / 1e12 if med[8] > 0 else None)
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
    if sys.argv[1:]:
        with open(sys.argv[1], "w") as f:
            json.dump({"rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
