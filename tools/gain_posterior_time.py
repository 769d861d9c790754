#!/usr/bin/env python3
"""cafe_gain_posterior next to cafe_score_per_family_gain on the same family lists.

    python tools/gain_posterior_time.py [OUT.json]     (on a machine with the GPU)

One process.  The two lists DESIGN section 8 quotes for the gain entry: the distinct families of the mammals table (order 141)
and 3000 families of the bench table (100 taxa, order 751), every family under its own (lambda, mu = lambda, nu = 0.3 lambda),
root_absent 0.1, sum rule.  The two calls are alternated, host wall around each (both synchronise); median, minimum and maximum
of the repetitions after one warm-up pair.  The posterior call is timed without the optional whole distributions."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cafexp_amd import capi, problem as P, synth  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")


def read(name):
    with open(os.path.join(DATA, name)) as f:
        return f.read()


def alternated(name, pb, fam, lam_mid, reps):
    pr = P.Params(lambdas=np.array([lam_mid]), prior=P.prior_uniform(pb.max_root_family_size))
    lam = lam_mid * (0.5 + np.random.default_rng(1).random(len(fam)))
    nu = 0.3 * lam
    ctx = capi.Context(pb)
    times = {"cafe_score_per_family_gain": [], "cafe_gain_posterior": []}
    try:
        ctx.set_root_rule("sum")
        calls = {"cafe_score_per_family_gain": lambda: ctx.score_per_family_gain(pr, fam, lam, lam, nu, 0.1),
                 "cafe_gain_posterior": lambda: ctx.gain_posterior(pr, fam, lam, lam, nu, 0.1)}
        assert np.array_equal(calls["cafe_score_per_family_gain"](), calls["cafe_gain_posterior"]()["lnl"])
        for _ in range(reps):
            for what, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[what].append((time.perf_counter() - t0) * 1e3)
    finally:
        ctx.close()
    rows = []
    for what, t in times.items():
        rows.append(dict(table=name, families=len(fam), branches=pb.n_nodes - 1, matrix_order=pb.matrix_size, call=what, repetitions=reps,
                         median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)))
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps(dict(table=name, ratio_of_medians=rows[1]["median_ms"] / rows[0]["median_ms"])), flush=True)
    return rows


def main():
    species, ids, counts = P.read_family_table(read("mammal_gene_families.txt"))
    mammals = P.build_problem(P.parse_newick(read("mammals_tree.txt")), species, ids, counts)
    distinct = np.unique(mammals.counts, axis=0, return_index=True)[1]
    bench, _ = synth.make_problem(n_taxa=100, n_families=3000, max_count=600)
    rows = alternated("mammal_gene_families.txt, distinct families", mammals, np.sort(distinct), 0.005, 7) + \
        alternated("bench table (100 taxa, order 751)", bench, np.arange(bench.n_families), 0.002, 3)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump({"rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
