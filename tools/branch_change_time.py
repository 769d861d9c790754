"""cafe_branch_change beside cafe_marginal_reconstruct on one context: order 300 (M = 299, R = 250), 4 000 families over the
seven-taxon tree of tests/missing_ref.py (counts drawn as that file draws them: a family's largest count from 1 to 280, every
other cell within a quarter below it), base model.  Wall time of cafe_branch_change at max_change D = 4, 10 and 32 and of
cafe_marginal_reconstruct -- the call that runs the same passes -- alternately in one process, REPS times each (with the band returned, and with pmf=False), all times kept
(a call's first run pays for mapping its fresh workspace and output arrays); the medians are what DESIGN.md quotes.  Then one run
of each with profiling on: the summed HIP-event time of the band kernel's launches (cafe_debug_branch_change_band) and of the
GEMM launches (cafe_debug_marginal_gemm).  With a family count as first argument the same on the bench table (100 taxa, N = 751) at
D = 10 alone, three times.  One process, one GPU; writes profiles/branch_change_time.json (or the path given as second argument)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from cafexp_amd import capi, problem as P, synth

REPS = 5


def order_300_table(F=4000, seed=2024):
    import missing_ref as MS
    M, R, cap = MS.SHAPES[300]
    rng = np.random.default_rng(seed)
    d = 1 + (np.arange(F) * cap) // F
    low = np.maximum(0, d - np.maximum(2, d // 4))
    counts = rng.integers(low[:, None], d[:, None] + 1, size=(F, len(MS.SPECIES))).astype(np.int32)
    counts[:, MS.SPECIES.index("D")] = d
    pb = P.build_problem(P.parse_newick(MS.NEWICK), MS.SPECIES, ["f%d" % i for i in range(F)], counts, root_filter=False,
                         max_family_size=M, max_root_family_size=R)
    return pb, P.Params(lambdas=MS.LAMBDA1.copy(), prior=P.prior_uniform(R))


def measure(table, pb, pr, Ds, reps=REPS):
    ctx = capi.Context(pb)
    ctx.score(pr)
    wall = {("change", D): [] for D in Ds}
    wall.update({("lean", D): [] for D in Ds})             # pmf=False: the bands stay on the device
    wall["marginal"] = []
    for _ in range(reps):                                    # alternately
        for D in Ds:
            t = time.perf_counter()
            got = ctx.branch_change(pr, max_change=D)
            wall[("change", D)].append(time.perf_counter() - t)
            failed = int(got["failed"].sum())
            del got
            t = time.perf_counter()
            ctx.branch_change(pr, max_change=D, pmf=False)
            wall[("lean", D)].append(time.perf_counter() - t)
        t = time.perf_counter()
        marg = ctx.marginal_reconstruct(pr)
        wall["marginal"].append(time.perf_counter() - t)
        del marg
    ctx.set_profiling(True)
    prof = {}
    for D in Ds:
        ctx.branch_change(pr, max_change=D, pmf=False)
        gemm_ms, gemm_flops = ctx.marginal_gemm_stats()
        prof[D] = {"band_ms": ctx.branch_change_band_ms(), "gemm_ms": gemm_ms, "gemm_flops": gemm_flops}
    ctx.marginal_reconstruct(pr)
    mms, mfl = ctx.marginal_gemm_stats()
    ctx.set_profiling(False)
    nI = int((pb.leaf_taxon < 0).sum())
    rec = {"table": table, "families": pb.n_families, "unique_families": int(ctx.stats()["n_unique_families"]), "nodes": pb.n_nodes,
           "interior_branches": nI - 1, "matrix_order": pb.matrix_size, "failed": failed, "marginal_reconstruct_seconds": wall["marginal"],
           "marginal_reconstruct_median_ms": 1e3 * float(np.median(wall["marginal"])), "marginal_reconstruct_gemm": {"ms": mms, "flops": mfl}, "branch_change": []}
    for D in Ds:
        s = wall[("change", D)]
        # the band kernel's arithmetic: two multiplies and one add per (column, interior branch, d, i), three flops per product
        flops = 3.0 * (2 * D + 1) * pb.max_family_size * (nI - 1) * rec["unique_families"]
        rec["branch_change"].append({"max_change": D, "seconds": s, "median_ms": 1e3 * float(np.median(s)),
                                     "without_pmf_seconds": wall[("lean", D)], "without_pmf_median_ms": 1e3 * float(np.median(wall[("lean", D)])), "band_kernel_ms": prof[D]["band_ms"],
                                     "band_kernel_gflops": flops / prof[D]["band_ms"] * 1e-6 if prof[D]["band_ms"] else None,
                                     "gemm_ms": prof[D]["gemm_ms"], "gemm_flops": prof[D]["gemm_flops"]})
    print(json.dumps(rec), flush=True)
    ctx.close()
    return rec


def main():
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "branch_change_time.json")
    runs = [measure("order 300, seven taxa", *order_300_table(), (4, 10, 32))]
    if len(sys.argv) > 1 and int(sys.argv[1]) > 0:
        pb, _ = synth.make_problem(n_families=int(sys.argv[1]))
        runs.append(measure("bench", pb, P.Params(lambdas=np.array([0.002]), prior=P.prior_uniform(pb.max_root_family_size)), (10,), reps=3))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": "AMD Instinct MI355X", "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
