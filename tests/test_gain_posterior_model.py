"""cafe_gain_posterior on the CPU: the numpy down pass of tests/gain_posterior_ref.py against the enumeration of every interior
size assignment, what the tables of the GPU test (tests/test_gain_posterior_gpu.py) can tell apart, and the header and the
exports."""
import os

import numpy as np
import pytest

import bd_lm_ref as R
import gain_posterior_ref as GP
import gain_ref as G
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_gain_model import six_taxon_rates
from test_per_family_shapes import TREE3, sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT_ABSENT = 0.2


def three_taxon(n):
    M, Rr = sizes(n)
    return _explicit_problem(TREE3, GP.patchy_families(n, M), M, Rr)


def rates3(pb):
    pick = np.arange(pb.n_families) % 4
    return G.RATES3[pick, :1], G.RATES3[pick, 1:2], G.RATES3[pick, 2:]


def _against_enumeration(pb, prior, lam, mu, nu, error_model=None):
    worst = 0.0
    for f in range(pb.n_families):
        mats = G.matrices(pb, lam[f], mu[f], nu[f])
        for absent in (0.0, ROOT_ABSENT):
            got = GP.down_pass(pb, pb.counts[f], mats, prior, absent, error_model)
            want = GP.enumerate_all(pb, pb.counts[f], mats, prior, absent, error_model)
            assert abs(got["lnl"] - want["lnl"]) <= 1e-12 * abs(want["lnl"])
            for key in GP.KEYS:
                assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
                worst = max(worst, np.nanmax(np.abs(got[key] - want[key])))
    print("largest difference between down pass and enumeration %.3e" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("n", [3, 16, 17])
def test_the_down_pass_is_the_enumeration_on_the_three_taxon_tree(n):
    pb = three_taxon(n)
    _against_enumeration(pb, P.prior_uniform(sizes(n)[1]), *rates3(pb))


def small_six_taxon(error=False, missing=False):
    """bd_lm_ref's tree and lambda tree at M = 5, R = 4: four interior nodes, 5 * 6^3 assignments"""
    counts = np.array([[1, 2, 1, 0, 2, 1], [0, 0, 1, 2, 1, 0], [3, 2, 0, 0, 0, 4], [0, 0, 0, 0, 0, 2]], dtype=np.int32)
    tokens = {}
    if missing:
        counts[0, 0] = counts[1, 3] = counts[2, 5] = P.COUNT_MISSING      # a cherry leaf, a leaf of the trifurcation, the leaf under the root
        tokens = dict(missing_tokens=("NA",))
    return P.build_problem(P.parse_newick(R.NEWICK), R.SPECIES, ["f%d" % i for i in range(4)], counts,
                           lambda_tree=P.parse_newick(R.LAMBDA_TREE, lambda_tree=True), root_filter=False, max_family_size=5,
                           max_root_family_size=4, n_deviations=3 if error else 0, **tokens)


@pytest.mark.parametrize("error,missing", [(False, False), (True, False), (False, True)])
def test_the_down_pass_is_the_enumeration_on_the_six_taxon_tree(error, missing):
    """A trifurcation, a leaf under the root, two lambda indices, the Poisson row 0; a 3-tap error model; missing cells (whose
    factor is the untruncated 1.0 in both)."""
    pb = small_six_taxon(error, missing)
    assert pb.matrix_size == 6 and pb.n_lambdas == 2
    lam, mu, nu = six_taxon_rates(pb)
    lam, mu, nu = 3 * lam, 3 * mu, 3 * nu                    # short tree, small sizes: rates at which the sizes move
    em = R.params(pb, "error").error_model if error else None
    _against_enumeration(pb, P.prior_poisson(4, 1.5), lam, mu, nu, em)


def _informative(values):
    return np.sum(np.any((values >= 0.05) & (values <= 0.95), axis=1))


@pytest.mark.parametrize("n", [17, 129, 641])
def test_the_three_taxon_tables_are_informative_and_tell_the_wrong_passes_apart(n):
    """At least one family with p_gain in [0.05, 0.95] on some branch and one with p_loss there; every wrong variant of the
    down pass moves some output by more than 1e-3, far above the GPU test's 1e-10."""
    pb = three_taxon(n)
    prior = P.prior_uniform(sizes(n)[1])
    lam, mu, nu = rates3(pb)
    fam = np.arange(pb.n_families)
    right = GP.table(pb, fam, lam, mu, nu, prior, ROOT_ABSENT)
    gains, losses = _informative(right["p_gain"]), _informative(right["p_loss"])
    print("n %d: %d families with an informative p_gain, %d with an informative p_loss" % (n, gains, losses))
    assert gains >= 1 and losses >= 1
    assert np.allclose(right["posterior"].sum(axis=2), 1.0, rtol=0, atol=1e-12)
    _wrong_variants_move(pb, fam, lam, mu, nu, prior, right)


def _wrong_variants_move(pb, fam, lam, mu, nu, prior, right, error_model=None):
    for which in GP.WRONG:
        wrong = GP.table(pb, fam, lam, mu, nu, prior, ROOT_ABSENT, error_model, wrong=which)
        moved = max(np.nanmax(np.abs(wrong[k] - right[k])) for k in GP.KEYS)
        print("%s: largest change of an output %.3e" % (which, moved))
        assert moved > 1e-3, which


@pytest.mark.parametrize("error", [False, True])
def test_the_six_taxon_table_tells_the_wrong_passes_apart(error):
    pb = R.problem(41, n_dev=3 if error else 0)
    pr = R.params(pb, "error" if error else "base")
    lam, mu, nu = six_taxon_rates(pb)
    fam = np.concatenate([np.arange(pb.n_families), [-1]])
    lam, mu, nu = (np.concatenate([x, x[2:3]]) for x in (lam, mu, nu))
    right = GP.table(pb, fam, lam, mu, nu, pr.prior, ROOT_ABSENT, pr.error_model)
    assert np.allclose(right["posterior"].sum(axis=2), 1.0, rtol=0, atol=1e-12)
    _wrong_variants_move(pb, fam, lam, mu, nu, pr.prior, right, pr.error_model)


def test_the_reports_arithmetic_and_text():
    """cafexp_amd/host/gain_origins_tests (no HIP library): the weighted sums, the p_gain > 0.5 counts, failed entries, both files"""
    import subprocess
    host = os.path.join(ROOT, "cafexp_amd", "host")
    mk = subprocess.run(["make", "-s", "-C", host, "gain_origins_tests"], capture_output=True, text=True)      # (incremental: never a stale program)
    assert mk.returncode == 0, mk.stderr[-2000:]
    out = subprocess.run([os.path.join(host, "gain_origins_tests")], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_the_entry_is_exported_and_declared():
    from cafexp_amd import capi
    lib = capi.load()
    assert lib.cafe_abi_version() == 3
    assert "cafe_gain_posterior" in capi.EXPORTS
    getattr(lib, "cafe_gain_posterior")
    header = open(os.path.join(ROOT, "include", "cafe_mi355x.h")).read()
    assert "#define CAFE_ABI_VERSION 3" in header
    assert "int cafe_gain_posterior(" in header and "} cafe_gain_posterior_out;" in header
    for field in ("lnl", "p_absent", "mean", "p_gain", "p_loss", "posterior"):
        assert "double* %s;" % field in header[header.index("typedef struct cafe_gain_posterior_out"):header.index("} cafe_gain_posterior_out;")]
    assert "untruncated" in header                           # the rule for a missing leaf is written down
    assert hasattr(capi.Context, "gain_posterior")
    assert [name for name, _ in capi.CafeGainPosteriorOut._fields_] == ["lnl", "p_absent", "mean", "p_gain", "p_loss", "posterior"]
