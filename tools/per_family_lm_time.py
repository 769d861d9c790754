#!/usr/bin/env python3
"""The two-rate per-family kernel next to the lambda = mu one, and cafe_simulate_lm next to cafe_simulate.

    python tools/per_family_lm_time.py [OUT.json]     (on a machine with the GPU)

One process.  Per table (the mammals table, order 141; the 2000-family bench table, order 751: the shapes DESIGN section 8 quotes
for cafe_score_per_family) one evaluation of every family under its own rates, host wall around the call (it synchronises), minimum
and median of 10 calls after 2 warm-up calls: cafe_score_per_family, cafe_score_per_family_lm at mu = lambda, at mu = 0.7 lambda,
and the first again.  The like-for-like figure is the first one of the same process: its device code is the earlier commit's.
Then cafe_simulate and cafe_simulate_lm (mu = lambda, mu = 0.7 lambda) on the 100-taxon, 20 011-family case of
tests/test_simulate_replay.py.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cafexp_amd import capi, problem as P, synth  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


def timed(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(t), "median_ms": float(np.median(t))}


def evaluation_rows(name, pb, lam_mid):
    pr = P.Params(lambdas=np.array([lam_mid]), prior=P.prior_uniform(pb.max_root_family_size))
    lam = lam_mid * (0.5 + np.random.default_rng(1).random(pb.n_families))
    fam = np.arange(pb.n_families)
    ctx = capi.Context(pb)
    rows = []
    try:
        assert np.array_equal(ctx.score_per_family(pr, fam, lam), ctx.score_per_family_lm(pr, fam, lam, lam))
        for what, fn in (("cafe_score_per_family", lambda: ctx.score_per_family(pr, fam, lam)),
                         ("cafe_score_per_family_lm, mu = lambda", lambda: ctx.score_per_family_lm(pr, fam, lam, lam)),
                         ("cafe_score_per_family_lm, mu = 0.7 lambda", lambda: ctx.score_per_family_lm(pr, fam, lam, 0.7 * lam)),
                         ("cafe_score_per_family again", lambda: ctx.score_per_family(pr, fam, lam))):
            row = dict(table=name, families=pb.n_families, matrix_order=pb.matrix_size, call=what, **timed(fn))
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        ctx.close()
    return rows


def simulate_rows():
    from test_simulate_replay import bench_case
    case = bench_case()
    kw = dict(chunk_size=case["chunk_size"], chunk_multiplier=case["chunk_multiplier"], error_model=case["error_model"],
              error_model_max_size=case["S"])
    lam = case["lambdas"]
    rows = []
    for what, fn in (("cafe_simulate", lambda: capi.simulate(case["tree"], lam, case["S"], case["roots"], seed=case["seed"], **kw)),
                     ("cafe_simulate_lm, mu = lambda", lambda: capi.simulate_lm(case["tree"], lam, lam, case["S"], case["roots"], seed=case["seed"], **kw)),
                     ("cafe_simulate_lm, mu = 0.7 lambda",
                      lambda: capi.simulate_lm(case["tree"], lam, [0.7 * v for v in lam], case["S"], case["roots"], seed=case["seed"], **kw))):
        row = dict(case="100 taxa, 20011 families, 47 chunks, S = 100, error model", call=what, **timed(fn))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    species, ids, counts = P.read_family_table(read("mammal_gene_families.txt"))
    mammals = P.build_problem(P.parse_newick(read("mammals_tree.txt")), species, ids, counts)
    bench, _ = synth.make_problem(n_taxa=100, n_families=2000, max_count=600)
    rows = evaluation_rows("mammal_gene_families.txt", mammals, 0.005) + \
        evaluation_rows("bench table (100 taxa, order 751), 2000 families", bench, 0.002) + simulate_rows()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump({"rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
