"""Times of the root rules at the bench shape (bench.py's default problem: 50 000 families, 100 taxa, gamma K = 8), one process:
cafe_score under CAFE_ROOT_MAX and CAFE_ROOT_SUM alternated, cafe_root_posterior, and cafe_marginal_reconstruct on the same
table.  Wall time of the synchronous call, median of --reps after one warm-up of each.  Prints one JSON line per figure and
appends them to --out (default profiles/root_rule_time.json, one JSON object per line).

    python tools/root_rule_time.py [--families N] [--taxa T] [--categories K] [--reps 3] [--no-marginal]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=50000)
    ap.add_argument("--taxa", type=int, default=100)
    ap.add_argument("--max-count", type=int, default=600)
    ap.add_argument("--categories", type=int, default=8)
    ap.add_argument("--lam", type=float, default=0.002)
    ap.add_argument("--alpha", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-marginal", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "root_rule_time.json"))
    args = ap.parse_args()

    import numpy as np
    from cafexp_amd import capi, problem as P, synth
    from cafexp_amd.gamma_rates import discrete_gamma

    pb, _ = synth.make_problem(n_taxa=args.taxa, n_families=args.families, max_count=args.max_count)
    K = args.categories
    pr = P.Params(lambdas=np.array([args.lam]), prior=P.prior_uniform(pb.max_root_family_size))
    if K > 1:
        pr.cat_probs, pr.multipliers = discrete_gamma(K, args.alpha)
    ctx = capi.Context(pb, max_categories=max(1, K))
    shape = {"families": pb.n_families, "taxa": args.taxa, "categories": K, "matrix_size": pb.matrix_size, "R": pb.max_root_family_size}

    def timed(fn):
        t0 = time.perf_counter()
        value = fn()
        return time.perf_counter() - t0, value

    seconds = {"max": [], "sum": []}
    values = {}
    for rule in ("max", "sum"):                              # warm-up
        ctx.set_root_rule(rule)
        ctx.score(pr, alpha=args.alpha)
    for _ in range(args.reps):                               # alternated
        for rule in ("max", "sum"):
            ctx.set_root_rule(rule)
            s, values[rule] = timed(lambda: ctx.score(pr, alpha=args.alpha))
            seconds[rule].append(s)
    ctx.set_root_rule("max")
    lines = [dict(shape, what="cafe_score", root_rule=rule, seconds=statistics.median(seconds[rule]), all_seconds=seconds[rule],
                  neg_lnl=values[rule]) for rule in ("max", "sum")]
    ctx.root_posterior(pr, alpha=args.alpha)
    post = [timed(lambda: ctx.root_posterior(pr, alpha=args.alpha)) for _ in range(args.reps)]
    res = post[-1][1]
    lines.append(dict(shape, what="cafe_root_posterior", seconds=statistics.median(s for s, _ in post), all_seconds=[s for s, _ in post],
                      n_used=res["n_used"], sum_of_total=float(res["total"].sum())))
    if not args.no_marginal:
        s, marg = timed(lambda: ctx.marginal_reconstruct(pr, alpha=args.alpha))
        ok = marg["failed"] == 0
        worst = float(np.max(np.abs(marg["log_evidence"][ok] - res["log_evidence"][ok]) / np.abs(marg["log_evidence"][ok])))
        lines.append(dict(shape, what="cafe_marginal_reconstruct", seconds=s, worst_relative_log_evidence_difference=worst))
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
