"""cafe_score_gradient beside cafe_marginal_reconstruct on one context of the bench table (50 000 families, 100 taxa,
N = 751): wall time of each call, run alternately in one process with the same parameters, base model and gamma K = 8,
with lambda = mu (one free rate per branch) and with death rates set (two: what the second free rate costs).  Every call
is timed REPS times and all times are kept (a call's first run pays for mapping its fresh workspace); the ratio is between
the medians.  Also the GEMM flops of both calls (cafe_debug_marginal_gemm).  One process, one GPU; writes
profiles/gradient_time.json (or the path given after the family count).

    python tools/gradient_time.py [FAMILIES [OUT.json]]
    python tools/gradient_time.py --one-call [FAMILIES]     one base-model gradient call and nothing else, for a profiler:
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/gradient_time.py --one-call
    python tools/gradient_time.py --fold RESULTS.db OUT.json  adds the kernel summary of such a run (the profiler's database) to OUT.json"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

REPS = 3


def setup(F):
    from cafexp_amd import capi, problem as P, synth
    from cafexp_amd.gamma_rates import discrete_gamma
    pb, _ = synth.make_problem(n_families=F)
    base = P.Params(lambdas=np.array([0.002]), prior=P.prior_uniform(pb.max_root_family_size))
    gamma = P.Params(lambdas=np.array([0.002]), prior=base.prior)
    gamma.cat_probs, gamma.multipliers = discrete_gamma(8, 2.0)
    return pb, base, gamma, capi.Context(pb, max_categories=8)


def kernel_name(full):
    """'void cafe::(anonymous namespace)::marginal_gemm_kernel<0, false>(cafe::GemmParams)' -> 'marginal_gemm_kernel<0, false>'"""
    import re
    m = re.search(r"(\w+(?:<[^()]*>)?)\(", full.replace("(anonymous namespace)::", ""))
    return m.group(1) if m else full


def fold(database, path):
    """the top_kernels view of the profiler's database (microseconds) into OUT.json"""
    import sqlite3
    rows = sqlite3.connect(database).execute("select name, total_calls, total_duration, average, percentage from top_kernels").fetchall()
    keep = [{"kernel": kernel_name(n), "calls": c, "total_ms": round(t / 1e3, 3), "average_us": round(a, 1), "percent": round(p, 2)} for n, c, t, a, p in rows]
    with open(path) as f:
        doc = json.load(f)
    doc["kernel_stats_of_one_base_gradient_call"] = keep
    doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats -- python tools/gradient_time.py --one-call (lambda = mu, base model, CAFE_ROOT_MAX)"
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--fold":
        return fold(sys.argv[2], sys.argv[3])
    if len(sys.argv) > 1 and sys.argv[1] == "--one-call":
        pb, base, _, ctx = setup(int(sys.argv[2]) if len(sys.argv) > 2 else 50000)
        got = ctx.score_gradient(base, "max")
        print("one call: failed %d of %d" % (int(got["failed"].sum()), pb.n_families))
        ctx.close()
        return
    F = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "gradient_time.json")
    pb, base, gamma, ctx = setup(F)
    ctx.score(base)
    lines = []
    for rates, mus in (("lambda_eq_mu", None), ("death_rates", [0.0016])):
        ctx.set_death_rates(mus)
        for model, pr, alpha in (("base", base, 1.0), ("gamma_k8", gamma, 2.0)):
            grad_s, marg_s, flops = [], [], {}
            for _ in range(REPS):                            # alternately
                t = time.perf_counter()
                got = ctx.score_gradient(pr, "max", alpha=alpha)
                grad_s.append(time.perf_counter() - t)
                flops["gradient"] = ctx.marginal_gemm_stats()[1]
                failed = int(got["failed"].sum())
                del got
                t = time.perf_counter()
                marg = ctx.marginal_reconstruct(pr, alpha=alpha)
                marg_s.append(time.perf_counter() - t)
                flops["marginal"] = ctx.marginal_gemm_stats()[1]
                marginal_failed = int(marg["failed"].sum())
                del marg
            rec = {"model": model, "rates": rates, "free_rates_per_branch": 1 if mus is None else 2, "families": pb.n_families,
                   "unique_families": int(ctx.stats()["n_unique_families"]), "nodes": pb.n_nodes, "matrix_order": pb.matrix_size,
                   "score_gradient_seconds": grad_s, "marginal_reconstruct_seconds": marg_s,
                   "ratio": float(np.median(grad_s) / np.median(marg_s)), "gemm_flops": flops,
                   "gemm_flops_ratio": flops["gradient"] / flops["marginal"], "failed": failed, "marginal_failed": marginal_failed}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    ctx.close()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": "AMD Instinct MI355X", "runs": lines}, f, indent=1)


if __name__ == "__main__":
    main()
