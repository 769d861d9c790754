"""cafe_expected_events beside cafe_score_gradient with death rates set (the call with the same GEMM count: up 1 + down 1 + 2
per interior branch) on one context of the bench table (50 000 families, 100 taxa, N = 751): wall time of each call, run
alternately in one process with the same parameters and the sum rule, base model and gamma K = 8.  Every call is timed REPS
times and all times are kept (a call's first run pays for mapping its fresh workspace); the ratio is between the medians.
Also the GEMM flops of both calls (cafe_debug_marginal_gemm; expected ratio 1.00).  One process, one GPU; writes
profiles/events_time.json (or the path given after the family count).

    python tools/events_time.py [FAMILIES [OUT.json]]
    python tools/events_time.py --one-call [FAMILIES]     one base-model call with death rates set and nothing else, for a profiler:
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/events_time.py --one-call
    python tools/events_time.py --fold RESULTS.db OUT.json  adds the kernel summary of such a run (the profiler's database) to OUT.json"""
import json
import os
import sys
import time

import numpy as np

from gradient_time import REPS, ROOT, kernel_name, setup

MUS = [0.0016]


def fold(database, path):
    """the top_kernels view of the profiler's database (microseconds) into OUT.json, and the share of this call's own kernels"""
    import sqlite3
    rows = sqlite3.connect(database).execute("select name, total_calls, total_duration, average, percentage from top_kernels").fetchall()
    keep = [{"kernel": kernel_name(n), "calls": c, "total_ms": round(t / 1e3, 3), "average_us": round(a, 1), "percent": round(p, 2)} for n, c, t, a, p in rows]
    with open(path) as f:
        doc = json.load(f)
    doc["kernel_stats_of_one_base_events_call"] = keep
    doc["percent_in_events_and_gradient_kernels"] = round(sum(k["percent"] for k in keep if k["kernel"].startswith(("events_", "gradient_"))), 2)
    doc["kernel_stats_source"] = "rocprofv3 --kernel-trace --stats -- python tools/events_time.py --one-call (death rates set, base model)"
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--fold":
        return fold(sys.argv[2], sys.argv[3])
    if len(sys.argv) > 1 and sys.argv[1] == "--one-call":
        pb, base, _, ctx = setup(int(sys.argv[2]) if len(sys.argv) > 2 else 50000)
        ctx.set_death_rates(MUS)
        got = ctx.expected_events(base)
        print("one call: failed %d of %d" % (int(got["failed"].sum()), pb.n_families))
        ctx.close()
        return
    F = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "events_time.json")
    pb, base, gamma, ctx = setup(F)
    ctx.score(base)
    ctx.set_death_rates(MUS)
    lines = []
    for model, pr, alpha in (("base", base, 1.0), ("gamma_k8", gamma, 2.0)):
        ev_s, grad_s, flops = [], [], {}
        for _ in range(REPS):                                # alternately
            t = time.perf_counter()
            got = ctx.expected_events(pr, alpha=alpha)
            ev_s.append(time.perf_counter() - t)
            flops["events"] = ctx.marginal_gemm_stats()[1]
            failed = int(got["failed"].sum())
            turnover = float(np.nansum(got["gains"]) + np.nansum(got["losses"]))
            del got
            t = time.perf_counter()
            grad = ctx.score_gradient(pr, "sum", alpha=alpha)
            grad_s.append(time.perf_counter() - t)
            flops["gradient"] = ctx.marginal_gemm_stats()[1]
            gradient_failed = int(grad["failed"].sum())
            del grad
        rec = {"model": model, "rates": "death_rates", "families": pb.n_families, "unique_families": int(ctx.stats()["n_unique_families"]),
               "nodes": pb.n_nodes, "matrix_order": pb.matrix_size, "expected_events_seconds": ev_s, "score_gradient_seconds": grad_s,
               "ratio": float(np.median(ev_s) / np.median(grad_s)), "gemm_flops": flops, "gemm_flops_ratio": flops["events"] / flops["gradient"],
               "failed": failed, "gradient_failed": gradient_failed, "expected_events_in_the_table": turnover}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    ctx.close()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": "AMD Instinct MI355X", "runs": lines}, f, indent=1)


if __name__ == "__main__":
    main()
