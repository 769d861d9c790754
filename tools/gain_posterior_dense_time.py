#!/usr/bin/env python3
"""cafe_gain_posterior_dense (one shared rate set, the dense prune and its down pass) next to cafe_gain_posterior with the same
rates tiled.

    python tools/gain_posterior_dense_time.py [--scaled] [OUT.json]     (on a machine with the GPU; --scaled: cafe_set_gain_scaling on)

One process.  The two lists of DESIGN section 8: the distinct families of the mammals table (order 141, 7 repetitions) and 3000
families of the bench table (100 taxa, order 751, 3 repetitions), mu = lambda, nu = 0.3 lambda, root_absent 0.1.  The two calls
are alternated, host wall around each (both synchronise); median, minimum and maximum of the repetitions after one warm-up pair,
whose results are compared first: the largest relative difference of the four node outputs, and the entry, node and output
that carry it.  Neither call is asked for the optional whole distributions.  Then the kernel split of the
dense call from cafe_debug_gain_dense_posterior under profiling, and the issued TFLOP/s of its two GEMMs (the up GEMM's flops
are those cafe_score_gain issues on the same list)."""
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
KINDS = ("build", "product", "gemm", "root", "weights", "gemm_t", "interior", "leaf")


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


def alternated(name, pb, fam, lam, reps):
    pr = P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(pb.max_root_family_size))
    nu = 0.3 * lam
    tiled = [np.full(len(fam), x) for x in (lam, lam, nu)]
    ctx = capi.Context(pb)
    times = {"cafe_gain_posterior": [], "cafe_gain_posterior_dense": []}
    try:
        if SCALED:
            ctx.set_gain_scaling(True)
        calls = {"cafe_gain_posterior": lambda: ctx.gain_posterior(pr, fam, *tiled, 0.1),
                 "cafe_gain_posterior_dense": lambda: ctx.gain_posterior_dense(pr, fam, [lam], [lam], [nu], 0.1)}
        a, b = calls["cafe_gain_posterior"](), calls["cafe_gain_posterior_dense"]()
        finite = np.isfinite(a["lnl"]) & np.isfinite(b["lnl"])
        assert SCALED or np.array_equal(np.isfinite(a["lnl"]), np.isfinite(b["lnl"]))   # (scaled: the dense call may be finite where the other is not)
        rel, where = 0.0, None
        for key in ("p_absent", "mean", "p_gain", "p_loss"):
            with np.errstate(invalid="ignore"):
                d = np.where(finite[:, None] & ~np.isnan(a[key]), np.abs(a[key] - b[key]) / np.maximum(np.abs(a[key]), 1e-290), 0.0)
            i, v = np.unravel_index(np.argmax(d), d.shape)
            if d[i, v] > rel:
                rel = float(d[i, v])
                where = dict(entry=int(i), family=int(fam[i]), node=int(v), output=key, cafe_gain_posterior=float(a[key][i, v]),
                             cafe_gain_posterior_dense=float(b[key][i, v]), lnl=float(a["lnl"][i]), counts_min=int(pb.counts[fam[i]].min()),
                             counts_max=int(pb.counts[fam[i]].max()))
        for _ in range(reps):
            for what, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[what].append((time.perf_counter() - t0) * 1e3)
        ctx.set_profiling(True)
        ctx.set_root_rule("sum")
        ctx.score_gain(pr, fam, [lam], [lam], [nu], 0.1)
        up_flops = ctx.gain_dense_profile()[1]
        split = []
        for _ in range(reps):
            calls["cafe_gain_posterior_dense"]()
            ms, flops = ctx.gain_dense_posterior_profile()
            split.append(list(ms) + [flops])
        ctx.set_profiling(False)
    finally:
        ctx.close()
    rows = []
    for what, t in times.items():
        rows.append(dict(table=name, families=len(fam), finite=int(finite.sum()), branches=pb.n_nodes - 1, matrix_order=pb.matrix_size, call=what,
                         repetitions=reps, median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)))
        print(json.dumps(rows[-1]), flush=True)
    med = np.median(np.array(split), axis=0)
    row = dict(table=name, scaled=SCALED, ratio_of_medians=rows[0]["median_ms"] / rows[1]["median_ms"], largest_relative_difference=rel,
               largest_difference_at=where)
    row.update({k + "_ms": float(v) for k, v in zip(KINDS, med)})
    row.update(gemm_tflops=up_flops / (med[2] * 1e-3) / 1e12 if med[2] > 0 else None,
               gemm_t_tflops=(med[8] - up_flops) / (med[5] * 1e-3) / 1e12 if med[5] > 0 else None)
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
