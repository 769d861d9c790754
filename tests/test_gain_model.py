"""The gene-gain model (birth-death with immigration) on the CPU: the numpy reference of tests/gain_ref.py against the matrix
exponential of the process's generator, the host helper cafe_bd_gain_row0 against 50-digit arithmetic, and what the tables of
the GPU test (tests/test_gain_gpu.py) can tell apart."""
import os
import subprocess

import numpy as np
import pytest

import bd_lm_ref as R
import gain_ref as G
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_per_family_shapes import TREE3, families, sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")


# lambda = mu, lambda > mu, lambda < mu
@pytest.mark.parametrize("lam,mu,nu,t", [(0.01, 0.01, 0.004, 30.0), (0.02, 0.012, 0.03, 25.0), (0.008, 0.015, 0.0005, 60.0)])
def test_the_reference_matrix_is_the_exponential_of_the_generator(lam, mu, nu, t):
    """Order 40 against expm of the generator truncated at order 400: what leaves the truncation by time t from a size below
    40 is far below the bound."""
    from scipy.linalg import expm
    got = G.matrix(40, lam, mu, nu, t)
    want = expm(G.generator(400, lam, mu, nu) * t)[:40, :40]
    worst = np.abs(got - want).max()
    print("lambda %g mu %g nu %g t %g: largest difference %.3e" % (lam, mu, nu, t, worst))
    assert worst <= 1e-12
    assert got[0, 1:].max() > 1e-3                           # row 0 is not e_0


def _row0_mp(lam, mu, nu, t, n):
    import mpmath as mp
    lq, mq, tq = (mp.mpf(int(lam * 1000000000)) / 1000000000, mp.mpf(int(mu * 1000000000)) / 1000000000, mp.mpf(int(t * 1000)) / 1000)
    nq = mp.mpf(int(nu * 1000000000)) / 1000000000
    if lq == 0:
        m = nq * tq if mq == 0 else nq * (1 - mp.exp(-mq * tq)) / mq
        return [mp.exp(-m) * m ** k / mp.factorial(k) for k in range(n)]
    if lq == mq:
        beta = lq * tq / (1 + lq * tq)
    else:
        E = mp.exp((lq - mq) * tq)
        beta = lq * (E - 1) / (lq * E - mq)
    r = nq / lq
    return [mp.binomial(r + k - 1, k) * (1 - beta) ** r * beta ** k for k in range(n)]


# r = 1e-6, 0.3, 1, 50; r = 500 and 1e9 (the series branch); lambda = 0 with and without deaths
ROW0_KEYS = [(0.01, 0.007, 1e-8, 30.0), (0.01, 0.007, 0.003, 30.0), (0.01, 0.01, 0.01, 30.0), (0.0002, 0.01, 0.01, 30.0),
             (0.0002, 0.01, 0.1, 30.0), (1e-9, 0.01, 1.0, 30.0), (0.0, 0.01, 0.02, 30.0), (0.0, 0.0, 0.02, 30.0)]


@pytest.mark.parametrize("lam,mu,nu,t", ROW0_KEYS)
def test_the_host_helper_against_fifty_digits(lam, mu, nu, t):
    """The helper works in the logarithm: five terms, the largest about lgamma(r + k) <= 450 for k < 64 and r <= 50 (the keys
    with larger r take the series, whose terms are of the size of k), each good to a few ulp: 450 * 2.2e-16 * 10 = 1e-12
    relative in the value."""
    import mpmath as mp
    from cafexp_amd import capi
    mp.mp.dps = 50
    n = 64
    got, r = capi.bd_gain_row0(lam, mu, nu, t, n)
    want = _row0_mp(lam, mu, nu, t, n)
    assert r == (np.inf if lam == 0 else G.quantize(nu) / G.quantize(lam))
    rel = max(float(abs(mp.mpf(float(g)) - w) / w) for g, w in zip(got, want) if w > 1e-290)
    print("r %g: largest relative difference %.3e, mass %.6f" % (r, rel, got.sum()))
    assert rel <= 1e-12
    if r <= 50 or lam == 0:                                  # the numpy reference states the same law (its gammaln difference cancels at large r)
        assert np.allclose(got, G.row0(n, lam, mu, nu, t), rtol=1e-11, atol=0)


def test_no_gain_is_exactly_the_unit_row():
    from cafexp_amd import capi
    for lam, mu, nu, t in [(0.01, 0.02, 0.0, 30.0), (0.01, 0.01, 0.0, 5.0), (0.0, 0.01, 0.0, 5.0), (0.01, 0.02, 0.9e-9, 30.0), (0.01, 0.02, 0.5, 0.0004)]:
        got, r = capi.bd_gain_row0(lam, mu, nu, t, 17)       # (a nu below the quantum, and a branch of quantized length 0, too)
        assert got[0] == 1.0 and not got[1:].any(), (lam, mu, nu, t, got)
    assert capi.bd_gain_row0(0.01, 0.02, 0.0, 30.0, 4)[1] == 0.0
    with pytest.raises(capi.CafeError):
        capi.bd_gain_row0(0.01, 0.02, -0.001, 30.0, 4)


def _tell_apart(pb, prior, lam, mu, nu, error_model=None):
    right = {rule: G.prune(pb, prior, lam, mu, nu, 0.2, rule, error_model=error_model) for rule in ("max", "sum")}
    assert all(np.isfinite(v).all() for v in right.values())
    for which in G.WRONG:
        for rule in ("max", "sum"):
            wrong = G.prune(pb, prior, lam, mu, nu, 0.2, rule, error_model=error_model, wrong=which)
            both = np.isfinite(wrong)
            rel = np.abs(wrong[both] - right[rule][both]) / np.abs(right[rule][both])
            print("%s, %s rule: relative differences %s" % (which, rule, rel))
            assert both.sum() >= len(both) - 1 and np.all(rel > 1e-6), (which, rule, rel)


@pytest.mark.parametrize("n", [3, 33, 129])
def test_the_every_width_rates_tell_the_wrong_models_apart(n):
    """The four (lambda, mu, nu) of the every-width GPU test on its tree and families, at three of its orders: nu ignored,
    r = nu / mu, alpha in place of beta in row 0, and row 0 convolved into the rows s >= 1 as well each miss the right value
    of every family by more than 1e-6 relative, far above the GPU test's 1e-10."""
    M, Rr = sizes(n)
    pb = _explicit_problem(TREE3, families(n), M, Rr)
    _tell_apart(pb, P.prior_uniform(Rr), G.RATES3[:, :1], G.RATES3[:, 1:2], G.RATES3[:, 2:])


@pytest.mark.parametrize("error", [False, True])
def test_the_six_taxon_table_tells_them_apart(error):
    pb = R.problem(41, n_dev=3 if error else 0)
    pr = R.params(pb, "error" if error else "base")
    lam, mu, nu = six_taxon_rates(pb)
    _tell_apart(pb, pr.prior, lam, mu, nu, error_model=pr.error_model)


def six_taxon_rates(pb):
    """One (lambdas, mus, nus) per family of bd_lm_ref.problem, two lambda indices with DIFFERENT nu"""
    rng = np.random.default_rng(7 + pb.matrix_size)
    lam = R.LAMBDAS * rng.uniform(0.6, 1.5, size=(pb.n_families, 2))
    mu = R.MUS * rng.uniform(0.6, 1.5, size=(pb.n_families, 2))
    nu = np.array([0.004, 0.0009]) * rng.uniform(0.6, 1.5, size=(pb.n_families, 2))
    lam[0, 1] = 0.0                                          # family 0: no births on the branches of the second index, the Poisson row 0
    return lam, mu, nu


def test_the_entry_and_the_helper_are_exported():
    from cafexp_amd import capi
    lib = capi.load()
    assert lib.cafe_abi_version() == 3
    for name in ("cafe_score_per_family_gain", "cafe_bd_gain_row0"):
        assert name in capi.EXPORTS
        getattr(lib, name)
    assert capi.CAFE_FAMILY_ABSENT == -1
    header = open(os.path.join(ROOT, "include", "cafe_mi355x.h")).read()
    assert "#define CAFE_ABI_VERSION 3" in header and "#define CAFE_FAMILY_ABSENT (-1)" in header
    assert "int cafe_score_per_family_gain(" in header and "int cafe_bd_gain_row0(" in header
    assert hasattr(capi.Context, "score_per_family_gain")


REFUSED = [
    (["-k", "2"], "-k > 1 and -a are not supported with --gain / --estimate-gain"),
    (["-a", "0.7"], "-k > 1 and -a are not supported with --gain / --estimate-gain"),
    (["-b"], "-b is not supported with --gain / --estimate-gain"),
    (["--gpus", "2"], "--gpus is not supported with --gain / --estimate-gain"),
    (["--simulate", "10", "-l", "0.01"], "--simulate is not supported with --gain / --estimate-gain"),
    (["--pvalues", "100"], "--pvalues simulates without a gain rate"),
    (["--reconstruct"], "the reconstructions are not ported to the gain model"),
    (["--reconstruct-marginal"], "the reconstructions are not ported to the gain model"),
    (["--sample-histories", "10"], "the reconstructions are not ported to the gain model"),
    (["--standard-errors"], "the posterior reports are not ported to the gain model"),
    (["--expected-events"], "the posterior reports are not ported to the gain model"),
    (["--rate-shift-scan"], "the posterior reports are not ported to the gain model"),
    (["--leaf-predictive"], "the posterior reports are not ported to the gain model"),
    (["--branch-change"], "the posterior reports are not ported to the gain model"),
    (["--estimate-rootdist"], "the posterior reports are not ported to the gain model"),
    (["--search-batch", "4"], "--search-batch is not supported with --gain / --estimate-gain"),
    (["-e"], "-e without FILE (estimating epsilon) is not supported with --gain / --estimate-gain"),
    (["--gain", "0.001"], "--gain fixes the gain rate and --estimate-gain searches it: give one of the two"),
    (["--root-absent", "1.5"], "--root-absent: P0 must lie in [0, 1]"),
]


def test_the_driver_refuses_what_the_gain_model_does_not_combine_with(tmp_path):
    """At argument checking, with a reason, before anything is read or written (the files named do not exist)."""
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    common = ["-t", str(tmp_path / "no_tree.txt"), "-i", str(tmp_path / "no_families.txt"), "-o", str(tmp_path / "out"), "--estimate-gain"]
    for extra, message in REFUSED:
        r = subprocess.run([DRIVER] + common + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and message in r.stderr, (extra, r.stderr)
    for extra, message in ((["--root-absent", "0.2"], "--root-absent sets the root's mass at size 0 under the gain model"),
                           (["--gain-unconditional"], "--gain-unconditional belongs to the gain model"),
                           (["--gain", "-0.001"], "--gain: NU must not be negative")):
        r = subprocess.run([DRIVER] + common[:-1] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and message in r.stderr, (extra, r.stderr)
    assert not os.path.exists(str(tmp_path / "out"))
