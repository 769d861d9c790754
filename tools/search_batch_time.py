"""ms per cafe_score_batch of G = 2, 4, 8 points against ms per cafe_score of one, on one context and in one process: every shape
is warmed first, then the sides are alternated `rounds` times (default 7) of `reps` calls each (default 100); printed are the
median and the range of the rounds.  Shapes: the mammals fixture (matrix order 141) base and gamma K = 4; a synthetic table at
matrix order 300; with `--bench` also the bench shape (order 751, 50 000 families, base model, G = 2 and 4), where one call
already fills the device and a batch is expected to cost about G calls.  Every batch value is checked against the single call's
bits before anything is timed.
  --calls [--root CHECKOUT]   ms per cafe_score alone, graphs on and off, of that checkout's library: one JSON line (run it from a
                              shell loop that alternates two commits)
  --search                    wall time of cafexp_hip's whole search on the mammals table, base and -k 4, with and without
                              --search-batch 4, alternated, at one seed"""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--bench", action="store_true")
ap.add_argument("--calls", action="store_true", help="ms per cafe_score only (mammals base and gamma K = 4, graphs on and off): one JSON line")
ap.add_argument("--search", action="store_true", help="wall time of the driver's whole search with and without --search-batch 4")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose library is timed by --calls (another commit's, to alternate the two in one command)")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, args.root if args.calls else HERE)
import numpy as np

from cafexp_amd import capi, problem as P, synth
from cafexp_amd.gamma_rates import discrete_gamma

data = os.path.join(HERE, "tests", "golden", "data")
rd = lambda n: open(os.path.join(data, n)).read()


def mammals_problem():
    species, ids, counts = P.read_family_table(rd("mammal_gene_families.txt"))
    return P.build_problem(P.parse_newick(rd("mammals_tree.txt")), species, ids, counts)


if args.calls:                                                     # (a): what tools/mammals_calls.py times, as medians of rounds
    pb = mammals_problem()
    prior = P.prior_uniform(pb.max_root_family_size)
    probs, mult = discrete_gamma(4, 2.0)
    cases = [("base", P.Params(lambdas=np.array([0.01]), prior=prior), 1.0),
             ("gamma_k4", P.Params(lambdas=np.array([0.005]), prior=prior, multipliers=mult, cat_probs=probs), 2.0)]
    out = {"root": args.root}
    for graphs in (True, False):
        ctx = capi.Context(pb, max_categories=4)
        ctx.set_graphs(graphs)
        for name, pr, alpha in cases:
            for _ in range(10):
                v = ctx.score(pr, alpha=alpha)
            ms = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    ctx.score(pr, alpha=alpha)
                ms.append((time.perf_counter() - t0) / args.reps * 1e3)
            out["%s_graphs_%s" % (name, "on" if graphs else "off")] = {"ms": float(np.median(ms)), "lo": min(ms), "hi": max(ms), "neg_lnl": v}
        ctx.close()
    print(json.dumps(out))
    sys.exit(0)

if args.search:                                                    # (c): the driver's search, the two sides alternated
    exe = os.path.join(HERE, "cafexp_amd", "host", "cafexp_hip")
    base = [exe, "-s", "7", "-t", os.path.join(data, "mammals_tree.txt"), "-i", os.path.join(data, "mammal_gene_families.txt")]
    for label, extra in (("base", []), ("gamma -k 4", ["-k", "4"])):
        sides = {"sequential": [], "--search-batch 4": []}
        info = {}
        for _ in range(max(5, args.rounds)):
            for side, more in (("sequential", []), ("--search-batch 4", ["--search-batch", "4"])):
                t0 = time.perf_counter()
                p = subprocess.run(base + extra + more, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
                wall = time.perf_counter() - t0
                j = json.loads(p.stdout.splitlines()[-1])
                sides[side].append((j["search"]["seconds"], wall))
                info[side] = j["search"]
        assert info["sequential"]["score"] == info["--search-batch 4"]["score"] and info["sequential"]["scorer_calls"] == info["--search-batch 4"]["scorer_calls"]
        for side, v in sides.items():
            s_, w_ = np.array([x[0] for x in v]), np.array([x[1] for x in v])
            print("%-12s %-18s search %.3f s (%.3f .. %.3f)  process %.2f s (%.2f .. %.2f)  iterations %d, points consumed %d, batches %s, points scored %s"
                  % (label, side, np.median(s_), s_.min(), s_.max(), np.median(w_), w_.min(), w_.max(), info[side]["iterations"], info[side]["scorer_calls"],
                     info[side].get("batches", "-"), info[side].get("points_scored", "-")), flush=True)
    sys.exit(0)


def points(pb, G, lam, K):
    prior = P.prior_uniform(pb.max_root_family_size)
    pts, alphas = [], []
    for g in range(G):
        pr = P.Params(lambdas=np.array([lam * (1 + 0.01 * g)]), prior=prior)
        if K > 1:
            pr.cat_probs, pr.multipliers = discrete_gamma(K, 2.0 + 0.05 * g)
        pts.append(pr)
        alphas.append(2.0 + 0.05 * g)
    return pts, alphas


def measure(label, pb, lam, K, Gs, reps):
    ctx = capi.Context(pb, max_categories=max(Gs) * K)
    pts, alphas = points(pb, max(Gs), lam, K)
    sides = [("one call", lambda: ctx.score(pts[0], alpha=alphas[0]))]
    for G in Gs:
        sides.append(("batch of %d" % G, lambda G=G: ctx.score_batch(pts[:G], alphas=alphas[:G])))
    single = np.array([ctx.score(p, alpha=a) for p, a in zip(pts, alphas)])
    for G in Gs:
        assert ctx.score_batch(pts[:G], alphas=alphas[:G]).tobytes() == single[:G].tobytes(), (label, G)
    for _, fn in sides:                                            # warm every shape
        for _ in range(5):
            fn()
    ms = {name: [] for name, _ in sides}
    for _ in range(args.rounds):
        for name, fn in sides:
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    one = np.median(ms["one call"])
    for name, _ in sides:
        v = np.array(ms[name])
        print("%-44s %-11s %8.4f ms (%.4f .. %.4f)  = %.2f calls" % (label, name, np.median(v), v.min(), v.max(), np.median(v) / one), flush=True)
    ctx.close()


mammals = mammals_problem()
measure("mammals order %d base" % mammals.matrix_size, mammals, 0.01, 1, (2, 4, 8), args.reps)
measure("mammals order %d gamma K=4" % mammals.matrix_size, mammals, 0.005, 4, (2, 4, 8), args.reps)
mid, _ = synth.make_problem(n_taxa=12, n_families=4000, max_count=239, lam_sim=0.004, seed=3, root_cap=150)
measure("synthetic order %d, %d families base" % (mid.matrix_size, mid.n_families), mid, 0.004, 1, (2, 4, 8), args.reps)
if args.bench:
    big, _ = synth.make_problem()
    measure("bench shape order %d, %d families base" % (big.matrix_size, big.n_families), big, 0.002, 1, (2, 4), max(3, args.reps // 20))
