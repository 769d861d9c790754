"""cafexp_hip under separate birth and death rates, the two paths that lacked them: --simulate --mu (host and device sampler) and
-b --family-mu (fixed rates, or searched per family).  On mammals_24 with the mammals tree, like tests/test_bd_lm_driver.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from cafexp_amd import problem as P
from helpers import DATA
from test_lambda_per_family import parse_output, problem

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
TREE = ["-t", os.path.join(DATA, "mammals_tree.txt")]
FAMILIES = ["-i", os.path.join(DATA, "mammals_24.txt")]
FILES = ("simulation.txt", "simulation_truth.txt")

pytestmark = pytest.mark.gpu


def _run(args, out, timeout=300):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([DRIVER] + args + ["-o", str(out)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _files(out):
    return [open(os.path.join(str(out), name), "rb").read() for name in FILES]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_simulate_under_the_pair(tmp_path, device):
    common = TREE + ["--simulate", "500", "-l", "0.0018", "-s", "7"] + (["--simulate-device"] if device else [])
    plain = _run(common, tmp_path / "plain")
    pair = _run(common + ["--mu", "0.0012"], tmp_path / "pair")
    same = _run(common + ["--mu", "0.0018"], tmp_path / "same")
    assert "mu" not in plain and pair["mu"] == [0.0012] and pair["n_families"] == 500
    for name, text in zip(FILES, _files(tmp_path / "pair")):
        assert len(text.splitlines()) == 501, name
    assert _files(tmp_path / "pair") != _files(tmp_path / "plain")       # the flag means something
    assert _files(tmp_path / "same") == _files(tmp_path / "plain")       # mu = lambda: byte for byte the run without it


@pytest.fixture(scope="module")
def lambda_only(tmp_path_factory):
    out = tmp_path_factory.mktemp("b")
    js = _run(TREE + FAMILIES + ["-b", "-s", "7"], out)
    assert "family_mu" not in js and not os.path.exists(os.path.join(str(out), "Base_mu_per_family.txt"))
    return parse_output(open(os.path.join(str(out), "Base_lambda_per_family.txt")).read())


def _rescore(lams, mus):
    """lnL of every family of mammals_24 under the reported rates (cafe_score_per_family_lm)"""
    from cafexp_amd import capi
    pb, _ = problem(families="mammals_24.txt")
    ctx = capi.Context(pb)
    try:
        return ctx.score_per_family_lm(P.Params(lambdas=np.ones(1), prior=P.prior_uniform(pb.max_root_family_size)),
                                       np.arange(pb.n_families), np.array(lams), np.array(mus))
    finally:
        ctx.close()


def test_family_mu_fixed(tmp_path, lambda_only):
    js = _run(TREE + FAMILIES + ["-b", "-s", "7", "--family-mu", "0.0012"], tmp_path)
    lam = parse_output((tmp_path / "Base_lambda_per_family.txt").read_text())
    mu = parse_output((tmp_path / "Base_mu_per_family.txt").read_text())
    assert js["family_mu"] == "fixed" and js["families"] == 24
    assert len(lam) == len(mu) == 24 and [r[0] for r in lam] == [r[0] for r in mu] == [r[0] for r in lambda_only]
    assert all(r[1] == [0.0012] for r in mu)
    assert [r[1] for r in lam] != [r[1] for r in lambda_only]            # another model, other optima


def test_family_mu_estimate_is_no_worse_than_lambda_only(tmp_path, lambda_only):
    js = _run(TREE + FAMILIES + ["-b", "-s", "7", "--family-mu", "estimate"], tmp_path)
    lam = parse_output((tmp_path / "Base_lambda_per_family.txt").read_text())
    mu = parse_output((tmp_path / "Base_mu_per_family.txt").read_text())
    assert js["family_mu"] == "estimate" and len(lam) == len(mu) == 24
    base_lam = [r[1] for r in lambda_only]
    lnl_pair = _rescore([r[1] for r in lam], [r[1] for r in mu])
    lnl_base = _rescore(base_lam, base_lam)
    print("lnL(lambda, mu) - lnL(lambda only) per family: %s" % (lnl_pair - lnl_base))
    assert np.all(np.isfinite(lnl_base))
    # nested models, and every search starts at mu = lambda (the tolerance of test_estimate_mu_is_no_worse...)
    assert np.all(-lnl_pair <= -lnl_base + 1e-6 * np.abs(lnl_base)), lnl_pair - lnl_base
    assert any(m[1] != l[1] for m, l in zip(mu, lam))


REFUSED = [
    (FAMILIES + ["--family-mu", "0.001"], "--family-mu sets the death rates of -b: it is not supported without -b"),
    (FAMILIES + ["-b", "--family-mu", "0.001", "-k", "2"], "-k > 1 and -a are not supported with it"),
    (["--simulate", "10", "-l", "0.002", "--estimate-mu"], "--estimate-mu is not supported with it"),
    (["--simulate", "10", "-l", "0.002", "--mu", "0.001,0.002"], "--mu needs one death rate per lambda (1)"),
]


@pytest.mark.parametrize("extra,message", REFUSED)
def test_flags_that_do_not_combine_are_refused(tmp_path, extra, message):
    r = subprocess.run([DRIVER] + TREE + extra + ["-o", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and message in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "out").exists()
