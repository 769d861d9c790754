"""cafexp_hip --standard-errors on synth20: with lambda searched, with -k 3 (lambda and alpha searched) and with
--estimate-mu (lambda and mu searched).  <Model>_standard_errors.txt parses, every SE is positive and equals, to 1e-8
relative, the square root of the diagonal of the inverse outer-product matrix computed in numpy from the binding's own
cafe_score_gradient scores (CAFE_ROOT_MAX) at the printed optimum, and |total score| is small against sqrt(trace I).
"Small": the searched objective is a sum over 96 families of maxima over the root size, smooth between the points where a
family's arg max changes; at its optimum the total score is zero up to the families that sit at such a point, a handful at
the most, and what the simplex search's stopping rule leaves.  sqrt(I_ii) is sqrt(96) ~ 10 typical scores, so half of it
is five families' worth: |U_i| <= 0.5 sqrt(I_ii) for every parameter."""
import json
import os
import subprocess

import numpy as np
import pytest

from cafexp_amd import problem as P
from helpers import DATA, read, table

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
COMMON = ["-t", os.path.join(DATA, "synth20_tree.txt"), "-i", os.path.join(DATA, "synth20_families.txt"), "-s", "7", "--standard-errors"]


def _parse(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# Standard errors") and lines[1].split("\t") == ["Parameter", "Estimate", "SE", "Lower95", "Upper95"]
    at_corr, at_score = lines.index("Correlation"), [i for i, ln in enumerate(lines) if ln.startswith("Total score")][0]
    rows = [ln.split("\t") for ln in lines[2:at_corr]]
    names = [r[0] for r in rows]
    table_ = np.array([[float(x) for x in r[1:]] for r in rows])
    corr = np.array([[float(x) for x in ln.split("\t")[1:]] for ln in lines[at_corr + 1:at_score]])
    score = np.array([float(ln.split("\t")[1]) for ln in lines[at_score + 1:at_score + 1 + len(names)]])
    assert lines[-1].startswith("# The errors are conditional on")
    return names, table_, corr, score


@pytest.mark.parametrize("extra,model,want", [([], "Base", ["Lambda"]), (["-k", "3"], "Gamma", ["Lambda", "Alpha"]),
                                              (["--estimate-mu"], "Base", ["Lambda", "Mu"])])
def test_standard_errors_are_the_inverse_outer_product_of_the_scores(tmp_path, extra, model, want):
    from cafexp_amd import capi
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([DRIVER] + COMMON + ["-o", str(tmp_path)] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    names, tab, corr, total = _parse(os.path.join(str(tmp_path), model + "_standard_errors.txt"))
    assert names == want == js["standard_errors"]["parameters"]
    est, se = tab[:, 0], tab[:, 1]
    assert np.all(se > 0) and np.all(np.isfinite(tab))
    assert np.allclose(tab[:, 2], est - 1.959963984540054 * se, rtol=1e-12) and np.allclose(tab[:, 3], est + 1.959963984540054 * se, rtol=1e-12)
    assert np.allclose(np.diag(corr), 1.0) and np.allclose(corr, corr.T, rtol=1e-9, atol=1e-12) and np.all(np.abs(corr) <= 1 + 1e-12)

    # the same scores from the binding at the printed optimum
    species, ids, counts = table("synth20_families.txt")
    pb = P.build_problem(P.parse_newick(read("synth20_tree.txt")), species, ids, counts)
    assert pb.n_families == js["n_families"] and pb.max_family_size == js["max_family_size"]
    pr = P.Params(lambdas=np.array(js["lambda"]), prior=P.prior_uniform(pb.max_root_family_size))
    K = 1
    if model == "Gamma":
        K = 3
        pr.multipliers, pr.cat_probs = np.array(js["multipliers"]), np.full(3, 1.0 / 3)
    ctx = capi.Context(pb, max_categories=K)
    try:
        if "mu" in js:
            ctx.set_death_rates(js["mu"])
        g = ctx.score_gradient(pr, "max", alpha=js.get("alpha", 1.0))
    finally:
        ctx.close()
    assert not g["failed"].any()
    cols = [g["d_lambda"][:, 0]]
    if "Mu" in want:
        cols.append(g["d_mu"][:, 0])
    if "Alpha" in want:
        cols.append(g["d_multiplier"] @ np.array(js["standard_errors"]["dmultiplier_dalpha"]))
    S = np.stack(cols, axis=1)
    info = S.T @ S
    cov = np.linalg.inv(info)
    want_se = np.sqrt(np.diag(cov))
    print(names, "SE", se, "numpy", want_se, "total score", total, "sqrt trace I", np.sqrt(np.trace(info)))
    assert np.all(np.abs(se - want_se) <= 1e-8 * want_se)
    assert np.allclose(total, S.sum(axis=0), rtol=1e-8, atol=1e-8 * np.sqrt(np.trace(info)))
    assert np.allclose(corr, cov / np.outer(want_se, want_se), rtol=1e-6, atol=1e-8)
    assert np.all(np.abs(total) <= 0.5 * np.sqrt(np.diag(info)))
