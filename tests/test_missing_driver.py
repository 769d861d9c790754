"""cafexp_hip on a table with missing cells: tests/golden/data/synth20_families_missing.txt is synth20_families.txt with 48 cells
spelled NA (our own fixture with cells blanked).

  * --missing NA fits a lambda that differs from the fit without the option (where atoi reads NA as an observed 0);
  * that fit is the Python path's: the binding scores the table read with missing_tokens at the printed lambda to the printed
    -lnL, and no lambda does better than the search's own tolerance allows (Nelder-Mead stops when the score moves less than
    1e-3: the printed -lnL is within 1e-3 of the minimum scipy finds, and lambda within the sqrt(2 * 1e-3 / f'') that allows);
  * --mask-cells of the same cells on the unblanked table writes the same results file;
  * --leaf-predictive writes <Model>_imputed_counts.tab, one line per missing cell, with the binding's mean and sd;
  * -b and --gpus 1 run on such a table; a combination that would reach a call without missing-cell support exits non-zero with
    its reason, before anything is read."""
import json
import os
import subprocess

import numpy as np
import pytest

from cafexp_amd import problem as P
from helpers import DATA, read

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
TREE = os.path.join(DATA, "synth20_tree.txt")
FULL = os.path.join(DATA, "synth20_families.txt")
BLANKED = os.path.join(DATA, "synth20_families_missing.txt")
SEARCH_TOL = 1e-3                                            # nelder_mead.cpp: the best score moving less than this ends the search


def _run(args, **kw):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    return subprocess.run([DRIVER] + args, capture_output=True, text=True, timeout=300, **kw)


def _json(r):
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _cells():
    """(family id, species) of the blanked cells, from the two golden tables"""
    sp, ids, blank = P.read_family_table(read("synth20_families_missing.txt"), missing_tokens=("NA",))
    _, _, full = P.read_family_table(read("synth20_families.txt"))
    assert blank.shape == full.shape and np.array_equal(blank[blank >= 0], full[blank >= 0])
    f, t = np.where(blank < 0)
    return [(ids[i], sp[j]) for i, j in zip(f, t)], sp, ids, blank


def test_the_golden_table_is_the_fixture_with_cells_blanked():
    cells, sp, ids, blank = _cells()
    assert len(cells) == 48 and len({c[0] for c in cells}) == 32
    assert P.max_sizes(blank) == P.max_sizes(P.read_family_table(read("synth20_families.txt"))[2])


@pytest.mark.gpu
def test_missing_na_is_fitted_as_unknown_and_agrees_with_the_python_path(tmp_path):
    from scipy.optimize import minimize_scalar
    from cafexp_amd import capi
    cells, sp, ids, blank = _cells()
    out, out0, out2 = str(tmp_path / "na"), str(tmp_path / "zero"), str(tmp_path / "mask")
    for d in (out, out0, out2):
        os.makedirs(d)                                       # (the driver writes into an existing -o directory)
    js = _json(_run(["-t", TREE, "-i", BLANKED, "-s", "7", "--missing", "NA", "-o", out]))
    js0 = _json(_run(["-t", TREE, "-i", BLANKED, "-s", "7", "-o", out0]))          # NA read as an observed 0
    lam, lam0 = js["lambda"][0], js0["lambda"][0]
    print("lambda with --missing NA %.9g, without %.9g" % (lam, lam0))
    assert abs(lam - lam0) > 0.05 * lam
    pb = P.build_problem(P.parse_newick(read("synth20_tree.txt")), None, None, read("synth20_families_missing.txt"), missing_tokens=("NA",))
    assert pb.missing_counts and pb.n_families == js["n_families"]
    assert (pb.max_family_size, pb.max_root_family_size) == (js["max_family_size"], js["max_root_family_size"])
    prior = P.prior_uniform(pb.max_root_family_size)
    ctx = capi.Context(pb)
    try:
        f = lambda x: ctx.score(P.Params(lambdas=np.array([x]), prior=prior))
        assert abs(f(lam) - js["neg_lnl"]) <= 1e-9 * abs(js["neg_lnl"])
        best = minimize_scalar(f, bounds=(lam / 3, lam * 3), method="bounded", options={"xatol": 1e-10})
        h = 0.02 * best.x
        curv = (f(best.x + h) - 2 * best.fun + f(best.x - h)) / h ** 2
    finally:
        ctx.close()
    print("python fit: lambda %.9g -lnL %.9g; driver %.9g %.9g; curvature %.4g" % (best.x, best.fun, lam, js["neg_lnl"], curv))
    assert -1e-6 <= js["neg_lnl"] - best.fun <= SEARCH_TOL
    assert curv > 0 and abs(lam - best.x) <= np.sqrt(2 * SEARCH_TOL / curv) + 1e-6
    with open(os.path.join(out, "Base_results.txt")) as fh:
        text = fh.read()
    assert "Missing cells: 48 in 32 families" in text
    with open(os.path.join(out0, "Base_results.txt")) as fh:
        assert "Missing cells" not in fh.read()                # without the option: the files of before

    # --mask-cells of the same cells on the unblanked table: the same results file
    mask = tmp_path / "mask.tab"
    mask.write_text("#FamilyID\tSpecies\tObserved\n" + "".join("%s\t%s\t0\tmore columns\n" % c for c in cells))
    js2 = _json(_run(["-t", TREE, "-i", FULL, "-s", "7", "--mask-cells", str(mask), "-o", out2]))
    assert js2["lambda"] == js["lambda"] and js2["neg_lnl"] == js["neg_lnl"]
    with open(os.path.join(out2, "Base_results.txt")) as fh:
        assert fh.read() == text
    with open(os.path.join(out, "Base_family_likelihoods.txt")) as a, open(os.path.join(out2, "Base_family_likelihoods.txt")) as b:
        assert a.read() == b.read()


@pytest.mark.gpu
def test_leaf_predictive_writes_one_imputed_line_per_missing_cell(tmp_path):
    from cafexp_amd import capi
    cells, sp, ids, blank = _cells()
    js = _json(_run(["-t", TREE, "-i", BLANKED, "-l", "0.01", "--missing", "NA", "--leaf-predictive", "-o", str(tmp_path)]))
    assert js["leaf_predictive"]["failed_cells"] == 0
    with open(os.path.join(str(tmp_path), "Base_imputed_counts.tab")) as fh:
        rows = [ln.rstrip("\n").split("\t") for ln in fh if ln.strip()]
    assert rows[0][:6] == ["#FamilyID", "Species", "Mean", "SD", "Lo95", "Hi95"]
    rows = rows[1:]
    pb = P.build_problem(P.parse_newick(read("synth20_tree.txt")), None, None, read("synth20_families_missing.txt"), missing_tokens=("NA",))
    kept = set(pb.family_ids)
    want = sorted(c for c in cells if c[0] in kept)
    assert sorted((r[0], r[1]) for r in rows) == want and len(rows) == len(want) == int((pb.counts < 0).sum())
    ctx = capi.Context(pb)
    try:
        got = ctx.leaf_predictive(P.Params(lambdas=np.array([0.01]), prior=P.prior_uniform(pb.max_root_family_size)))
    finally:
        ctx.close()
    for r in rows:
        f, t = pb.family_ids.index(r[0]), [x.lower() for x in pb.taxa].index(r[1].lower())
        assert pb.counts[f, t] < 0 and np.isnan(got["p_obs"][f, t])
        assert r[2] == "%.6g" % got["mean"][f, t] and r[3] == "%.6g" % got["sd"][f, t]
        lo, hi = int(r[4]), int(r[5])
        assert 0 <= lo <= got["mean"][f, t] <= hi
        assert lo == max(0, int(np.floor(got["mean"][f, t] - 1.959963984540054 * got["sd"][f, t])))
        assert hi == int(np.ceil(got["mean"][f, t] + 1.959963984540054 * got["sd"][f, t]))
    with open(os.path.join(str(tmp_path), "Base_leaf_predictive.tab")) as fh:
        body = fh.read()
    assert body.count(":NA:NA") == len(rows)


@pytest.mark.gpu
def test_per_family_and_sharded_runs_accept_missing_cells(tmp_path):
    js = _json(_run(["-t", TREE, "-i", BLANKED, "-l", "0.01", "--missing", "NA", "--gpus", "1"]))
    one = _json(_run(["-t", TREE, "-i", BLANKED, "-l", "0.01", "--missing", "NA"]))
    assert abs(js["neg_lnl"] - one["neg_lnl"]) <= 1e-12 * abs(one["neg_lnl"])
    r = _run(["-t", TREE, "-i", BLANKED, "--missing", "NA", "-b", "--limit", "12", "-s", "3", "-o", str(tmp_path)])
    assert r.returncode == 0, r.stderr
    with open(os.path.join(str(tmp_path), "Base_lambda_per_family.txt")) as fh:
        rows = [ln.split("\t") for ln in fh if ln.strip()]
    assert len(rows) == 12 and all(float(x[1].split()[-1].strip()) > 0 for x in rows)


@pytest.mark.parametrize("extra,word", [(["--pvalues", "10"], "--pvalues"), (["--reconstruct"], "--reconstruct"),
                                         (["--reconstruct-marginal"], "--reconstruct-marginal"), (["--sample-histories", "5"], "--sample-histories"),
                                         (["--standard-errors"], "--standard-errors"), (["--expected-events"], "--expected-events"),
                                         (["--rate-shift-scan"], "--rate-shift-scan")])
@pytest.mark.parametrize("option", [["--missing", "NA"], ["--mask-cells", "no_such_file"]])
def test_a_combination_that_reaches_a_refused_call_fails_at_argument_checking(extra, word, option):
    if not os.path.exists(DRIVER):
        pytest.fail("cafexp_hip missing: run __graft_entry__.build()")
    r = _run(["-t", TREE, "-i", BLANKED] + option + extra)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith("cafexp_hip: " + word) and "missing cells" in r.stderr or "--missing / --mask-cells" in r.stderr
    assert "no_such_file" not in r.stderr                        # refused before anything is read
