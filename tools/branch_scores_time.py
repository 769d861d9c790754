"""cafe_branch_scores beside cafe_score_gradient on one context of the bench table (50 000 families, 100 taxa, N = 751):
wall time of each call, run alternately in one process with the same parameters, base model and gamma K = 8, with
lambda = mu and with death rates set.  Every call is timed REPS times and all times are kept; the ratio is between the
medians.  cafe_branch_scores runs as the driver's --rate-shift-scan runs it (total and Gram matrix, nothing per family) and
once more with the per-family rows.  Also the GEMM flops of both calls (cafe_debug_marginal_gemm: equal), and the Gram
kernel's own HIP-event time and flops (cafe_debug_gram, profiling on for one extra call) against the fp64 MFMA peak DESIGN.md
quotes.  One process, one GPU; writes profiles/branch_scores_time.json (or the path given after the family count).

    python tools/branch_scores_time.py [FAMILIES [OUT.json]]
    python tools/branch_scores_time.py --one-call [FAMILIES]     one base-model call (Gram, no rows) and nothing else, for a profiler:
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/branch_scores_time.py --one-call
    python tools/branch_scores_time.py --fold RESULTS.db OUT.json  adds the kernel summary of such a run to OUT.json"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from gradient_time import kernel_name, setup

REPS = 3
PEAK_TFLOPS = 78.6                                           # fp64 MFMA peak of the MI355X


def fold(database, path):
    import sqlite3
    rows = sqlite3.connect(database).execute("select name, total_calls, total_duration, average, percentage from top_kernels").fetchall()
    keep = [{"kernel": kernel_name(n), "calls": c, "total_ms": round(t / 1e3, 3), "average_us": round(a, 1), "percent": round(p, 2)} for n, c, t, a, p in rows]
    with open(path) as f:
        doc = json.load(f)
    doc["kernel_stats_of_one_base_call"] = keep
    doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats -- python tools/branch_scores_time.py --one-call (lambda = mu, base model, CAFE_ROOT_MAX)"
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--fold":
        return fold(sys.argv[2], sys.argv[3])
    if len(sys.argv) > 1 and sys.argv[1] == "--one-call":
        pb, base, _, ctx = setup(int(sys.argv[2]) if len(sys.argv) > 2 else 50000)
        got = ctx.branch_scores(base, "max", per_family=False)
        print("one call: failed %d of %d, %d scores" % (int(got["failed"].sum()), pb.n_families, len(got["total"])))
        ctx.close()
        return
    F = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "branch_scores_time.json")
    pb, base, gamma, ctx = setup(F)
    ctx.score(base)
    lines = []
    for rates, mus in (("lambda_eq_mu", None), ("death_rates", [0.0016])):
        ctx.set_death_rates(mus)
        for model, pr, alpha in (("base", base, 1.0), ("gamma_k8", gamma, 2.0)):
            scan_s, rows_s, grad_s, flops = [], [], [], {}
            for _ in range(REPS):                            # alternately
                t = time.perf_counter()
                got = ctx.branch_scores(pr, "max", alpha=alpha, per_family=False)
                scan_s.append(time.perf_counter() - t)
                flops["branch_scores"] = ctx.marginal_gemm_stats()[1]
                failed, P = int(got["failed"].sum()), len(got["total"])
                del got
                t = time.perf_counter()
                grad = ctx.score_gradient(pr, "max", alpha=alpha)
                grad_s.append(time.perf_counter() - t)
                flops["gradient"] = ctx.marginal_gemm_stats()[1]
                del grad
                t = time.perf_counter()
                got = ctx.branch_scores(pr, "max", alpha=alpha, gram=False)
                rows_s.append(time.perf_counter() - t)
                del got
            ctx.set_profiling(True)
            ctx.branch_scores(pr, "max", alpha=alpha, per_family=False)
            gram_ms, gram_flops = ctx.gram_stats()
            ctx.set_profiling(False)
            tflops = gram_flops / (gram_ms * 1e9) if gram_ms > 0 else 0.0
            rec = {"model": model, "rates": rates, "families": pb.n_families, "unique_families": int(ctx.stats()["n_unique_families"]),
                   "nodes": pb.n_nodes, "matrix_order": pb.matrix_size, "scores": P, "panel_megabytes": P * (-(-int(ctx.stats()["n_unique_families"]) // 128) * 128) * 8 / 1e6,
                   "branch_scores_gram_only_seconds": scan_s, "branch_scores_rows_only_seconds": rows_s, "score_gradient_seconds": grad_s,
                   "ratio_gram_only": float(np.median(scan_s) / np.median(grad_s)), "ratio_rows_only": float(np.median(rows_s) / np.median(grad_s)),
                   "gemm_flops": flops, "gemm_flops_equal": flops["branch_scores"] == flops["gradient"],
                   "gram_ms": gram_ms, "gram_flops": gram_flops, "gram_tflops": tflops, "gram_fraction_of_fp64_mfma_peak": tflops / PEAK_TFLOPS, "failed": failed}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    ctx.close()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": "AMD Instinct MI355X", "fp64_mfma_peak_tflops": PEAK_TFLOPS, "runs": lines}, f, indent=1)


if __name__ == "__main__":
    main()
