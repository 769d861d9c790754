#!/usr/bin/env python3
"""Generates tests/golden/ref_magnitude_audit.json: the per-family values of the edge families of
tests/test_magnitude_audit.py by the CPU oracle with its EXACT matrices (fast=False, the reference's own sums).

    python tests/golden/make_magnitude_audit_golden.py

The test measures the oracle's fast-against-exact difference on these families and sets its tolerance from it.  The fast
side it computes itself; the exact matrices of order 751 take the oracle half a minute per call, which is why they are
recorded here.  The fixture holds the count rows the values belong to: the test refuses it when its own rows differ."""
import dataclasses
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
from oracle import oracle as O  # noqa: E402
from cafexp_amd import problem as P, synth  # noqa: E402
import magskip_ref as R  # noqa: E402

OUT = os.path.join(HERE, "ref_magnitude_audit.json")


def main():
    O.build()
    # the table of tests/test_magnitude_skip.py's _problem(600, n_families=248)
    pb0, _ = synth.make_problem(n_taxa=7, n_families=248, max_count=600, lam_sim=0.003, seed=5, root_cap=300, n_deviations=0)
    g = {"generator": "tests/golden/make_magnitude_audit_golden.py", "source": "oracle (fast=False)", "calls": {}}
    for call, (lam, gamma) in R.CALLS.items():
        pr = P.Params(lambdas=np.full(pb0.n_lambdas, lam), prior=P.prior_uniform(pb0.max_root_family_size))
        if gamma:
            pr.cat_probs, pr.multipliers = O.discrete_gamma(2, R.ALPHA)
        pb, idx, tops, _ = R.edge_problem(O, pb0, pr)
        sub = dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[idx]), family_ids=[pb.family_ids[i] for i in idx])
        e = {"lambda": lam, "gamma": gamma, "rows": sub.counts.tolist(), "largest_root_likelihood": tops.tolist()}
        if gamma:
            _, cat, fam = O.score_gamma(sub, pr, fast=False, per_family=True)
            e["category_likelihood"], e["family_likelihood"] = cat.tolist(), fam.tolist()
        else:
            e["family_lnl"] = O.score_base(sub, pr, fast=False, per_family=True)[1].tolist()
        g["calls"][call] = e
        print(call, "done", flush=True)
    with open(OUT, "w") as f:
        json.dump(g, f, indent=0, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
