"""cafexp_hip with separate birth and death rates: --estimate-mu searches lambda and mu together, --mu fixes mu, and a run
without either flag writes what the driver wrote before the flags existed (tests/golden/bd_lm_driver_parent.json: the files of
the same command line, recorded from the commit before them)."""
import json
import os
import subprocess

import pytest

from helpers import DATA

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
COMMON = ["-t", os.path.join(DATA, "mammals_tree.txt"), "-i", os.path.join(DATA, "mammals_24.txt"), "-s", "7"]

pytestmark = pytest.mark.gpu


def _run(extra, out):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    os.makedirs(str(out), exist_ok=True)
    r = subprocess.run([DRIVER] + COMMON + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), open(os.path.join(str(out), "Base_results.txt")).read()


@pytest.fixture(scope="module")
def lambda_only(tmp_path_factory):
    out = tmp_path_factory.mktemp("lambda_only")
    return _run([], out) + (out,)


def test_without_the_flags_the_files_are_the_parents(lambda_only):
    _, results, out = lambda_only
    with open(os.path.join(HERE, "golden", "bd_lm_driver_parent.json")) as f:
        golden = json.load(f)
    assert "Mu:" not in results
    for name, text in golden["files"].items():
        assert open(os.path.join(str(out), name)).read() == text, name


def test_estimate_mu_is_no_worse_than_lambda_only_and_reports_mu(lambda_only, tmp_path):
    base, _, _ = lambda_only
    js, results = _run(["--estimate-mu"], tmp_path)
    print("-lnL lambda only %.10f (lambda %r), lambda and mu %.10f (lambda %r, mu %r)"
          % (base["neg_lnl"], base["lambda"], js["neg_lnl"], js["lambda"], js["mu"]))
    # nested models, and the search starts at mu = lambda
    assert js["neg_lnl"] <= base["neg_lnl"] + 1e-6 * abs(base["neg_lnl"])
    lines = results.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("Lambda:")]
    assert len(at) == 1 and lines[at[0] + 1].startswith("Mu:")
    assert float(lines[at[0] + 1].split(":")[1]) == pytest.approx(js["mu"][0], rel=1e-12)
    assert len(js["mu"]) == 1 and js["mu"][0] >= 0 and js["mu"][0] != js["lambda"][0]


def test_fixed_mu_is_scored_and_reconstructed_under_the_pair(tmp_path):
    lam = 0.0018
    same, _ = _run(["-l", str(lam), "--mu", str(lam)], tmp_path / "same")
    plain, _ = _run(["-l", str(lam)], tmp_path / "plain")
    assert same["neg_lnl"] == plain["neg_lnl"]                       # mu = lambda: the lambda = mu bits
    other, results = _run(["-l", str(lam), "--mu", "0.0012", "--reconstruct", "--reconstruct-marginal", "--pvalues", "20"], tmp_path / "other")
    assert other["mu"] == [0.0012] and other["neg_lnl"] != plain["neg_lnl"]
    assert "Mu:" in results and other["marginal"]["failed"] == 0
    assert os.path.exists(str(tmp_path / "other" / "Base_posterior_sizes.tab"))


def test_flags_that_do_not_combine_are_refused(tmp_path):
    for extra, message in ((["--estimate-mu", "--mu", "0.001"], "give one of the two"),
                           (["--estimate-mu", "-l", "0.002"], "-l / -m are not supported with it"),
                           (["--mu", "0.001", "-b"], "--mu / --estimate-mu are not supported with it")):
        r = subprocess.run([DRIVER] + COMMON + ["-o", str(tmp_path / "out")] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and message in r.stderr, (extra, r.stderr)
