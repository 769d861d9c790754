"""cafe_leaf_predictive beside cafe_marginal_reconstruct on one context, at the bench table (50 000 families, 100 taxa, N = 751;
base model and gamma K = 8) and at the mammals example (base model): wall time of each call, run alternately in one process with
the same parameters.  Every call is timed REPS times and all times are kept (a call's first run pays for mapping its fresh
workspace and output arrays); the ratio is between the medians.  Then one run of each call with profiling on: the summed HIP-event
time and the flops of its GEMM launches (cafe_debug_marginal_gemm) and their rate.  cafe_marginal_reconstruct launches
marginal_gemm_kernel only; cafe_leaf_predictive launches it for the up pass and the interior branches of the down pass (two thirds
of the other call's flops) and predictive_gemm_kernel for the leaf branches, so the new kernel's own rate is estimated as
(flops - 2/3 marginal flops) / (ms - 2/3 marginal ms).  One process, one GPU; writes profiles/leaf_predictive_time.json (or the path
given after the family count)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from cafexp_amd import capi, problem as P, synth
from cafexp_amd.gamma_rates import discrete_gamma

REPS = 3
DATA = os.path.join(ROOT, "tests", "golden", "data")


def bench_table(F):
    pb, _ = synth.make_problem(n_families=F)
    base = P.Params(lambdas=np.array([0.002]), prior=P.prior_uniform(pb.max_root_family_size))
    gamma = P.Params(lambdas=np.array([0.002]), prior=base.prior)
    gamma.cat_probs, gamma.multipliers = discrete_gamma(8, 2.0)
    return pb, [("base", base, 1.0), ("gamma_k8", gamma, 2.0)], 8


def mammals():
    with open(os.path.join(DATA, "mammals_tree.txt")) as t, open(os.path.join(DATA, "mammal_gene_families.txt")) as f:
        tree, (species, ids, counts) = P.parse_newick(t.read()), P.read_family_table(f.read())
    pb = P.build_problem(tree, species, ids, counts)
    return pb, [("base", P.Params(lambdas=np.array([0.0018]), prior=P.prior_uniform(pb.max_root_family_size)), 1.0)], 1


def measure(table, pb, models, K):
    ctx = capi.Context(pb, max_categories=K)
    ctx.score(models[0][1])
    lines = []
    for model, pr, alpha in models:
        pred_s, marg_s = [], []
        for _ in range(REPS):                                # alternately
            t = time.perf_counter()
            got = ctx.leaf_predictive(pr, alpha=alpha)
            pred_s.append(time.perf_counter() - t)
            nan_cells, lpl = int(np.isnan(got["p_obs"]).sum()), float(np.log(got["p_obs"][got["p_obs"] > 0]).sum())
            del got
            t = time.perf_counter()
            marg = ctx.marginal_reconstruct(pr, alpha=alpha)
            marg_s.append(time.perf_counter() - t)
            marginal_failed = int(marg["failed"].sum())
            del marg
        ctx.set_profiling(True)
        ctx.leaf_predictive(pr, alpha=alpha)
        pms, pfl = ctx.marginal_gemm_stats()
        ctx.marginal_reconstruct(pr, alpha=alpha)
        mms, mfl = ctx.marginal_gemm_stats()
        ctx.set_profiling(False)
        leaf_ms, leaf_fl = pms - 2 * mms / 3, pfl - 2 * mfl / 3
        rec = {"table": table, "model": model, "families": pb.n_families, "unique_families": int(ctx.stats()["n_unique_families"]), "nodes": pb.n_nodes,
               "matrix_order": pb.matrix_size, "leaf_predictive_seconds": pred_s, "marginal_reconstruct_seconds": marg_s,
               "ratio": float(np.median(pred_s) / np.median(marg_s)), "nan_cells": nan_cells, "log_pseudo_likelihood": lpl, "marginal_failed": marginal_failed,
               "leaf_predictive_gemm": {"ms": pms, "flops": pfl, "tflops": pfl / pms * 1e-9 if pms else None},
               "marginal_reconstruct_gemm": {"ms": mms, "flops": mfl, "tflops": mfl / mms * 1e-9 if mms else None},
               "predictive_gemm_kernel_estimate": {"ms": leaf_ms, "flops": leaf_fl, "tflops": leaf_fl / leaf_ms * 1e-9 if leaf_ms > 0 else None}}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    ctx.close()
    return lines


def main():
    F = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "leaf_predictive_time.json")
    lines = measure("bench", *bench_table(F)) + measure("mammals", *mammals())
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": "AMD Instinct MI355X", "runs": lines}, f, indent=1)


if __name__ == "__main__":
    main()
