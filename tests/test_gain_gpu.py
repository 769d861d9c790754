"""cafe_score_per_family_gain (family_gain.hip, family_gain_kernel.h): the per-family kernel under a gene gain rate, root sizes
0..R.

Reference: the numpy prune of tests/gain_ref.py (tests/test_gain_model.py pins its matrices to the matrix exponential and shows
what these tables tell apart).  Tolerance: the per-family one, test_lambda_per_family._close at REL = 1e-10, infinities matched
exactly.  With nu = 0 and root_absent = 0 the values are compared with cafe_score_per_family_lm's and cafe_score_per_family's by
==.  A reference is computed once per table and shared by the rules and the root masses that read it."""
import numpy as np
import pytest

import bd_lm_ref as R
import gain_ref as G
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_gain_model import six_taxon_rates
from test_lambda_per_family import _close
from test_per_family_lm import EVERY_WIDTH
from test_per_family_shapes import ORDERS, TREE3, WIDTHS, families, sizes, width

RULES = ("max", "sum")
ABSENT = (0.0, 0.2)
LAM, MU, NU = G.RATES3[:, :1], G.RATES3[:, 1:2], G.RATES3[:, 2:]


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _every_rule_and_root_mass(ctx, pb, pr, fam, lam, mu, nu, vectors):
    """the call under both root rules and both root masses against the shared root vectors; returns the last values"""
    got = None
    try:
        for rule in RULES:
            ctx.set_root_rule(rule)
            for absent in ABSENT:
                got = ctx.score_per_family_gain(pr, fam, lam, mu, nu, absent)
                want = np.array([G.reduce_root(L, pr.prior, absent, rule) for L in vectors])
                print("%s rule, root_absent %g: " % (rule, absent), end="")
                _close(got, want)
    finally:
        ctx.set_root_rule("max")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", ORDERS)
def test_every_width_against_the_numpy_prune(capi, n):
    """One family of each kind, each under its own (lambda, mu, nu), either side of every switch of the width ladder."""
    M, Rr = sizes(n)
    pb = _explicit_problem(TREE3, families(n), M, Rr)
    assert pb.matrix_size == n and pb.n_families == 4
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    vectors = G.root_vectors(pb, LAM, MU, NU)
    ctx = capi.Context(pb)
    try:
        got = _every_rule_and_root_mass(ctx, pb, pr, np.arange(4), LAM, MU, NU, vectors)
    finally:
        ctx.close()
    print("n %d E %d: lnL %s" % (n, width(n), got))
    assert np.isfinite(got).all()


def _six_taxon(order, error, missing):
    pb = R.problem(order, n_dev=3 if error else 0)
    if missing:
        counts = pb.counts.copy()
        counts[0, 0] = counts[1, 3] = counts[2, 5] = counts[3, 1] = counts[3, 2] = P.COUNT_MISSING     # a cherry leaf, a leaf of the trifurcation, the leaf under the root
        pb = P.build_problem(P.parse_newick(R.NEWICK), R.SPECIES, list(pb.family_ids), counts, lambda_tree=P.parse_newick(R.LAMBDA_TREE, lambda_tree=True),
                             root_filter=False, max_family_size=pb.max_family_size, max_root_family_size=pb.max_root_family_size, missing_tokens=("NA",))
        assert pb.missing_counts and pb.matrix_size == order
    return pb


@pytest.mark.gpu
@pytest.mark.parametrize("order,error,missing", [(41, False, False), (300, False, False), (41, True, False), (41, False, True)])
def test_the_six_taxon_tree(capi, order, error, missing):
    """A trifurcation, a leaf under the root, two lambda indices with different nu, one family whose second lambda is 0 (the
    Poisson row 0), the all-zero profile as a listed family; with a 3-tap error model; with missing cells."""
    pb = _six_taxon(order, error, missing)
    pr = R.params(pb, "error" if error else "base")
    lam, mu, nu = six_taxon_rates(pb)
    fam = np.concatenate([np.arange(pb.n_families), [capi.CAFE_FAMILY_ABSENT]])
    lam, mu, nu = (np.concatenate([x, x[2:3]]) for x in (lam, mu, nu))
    assert lam[0, 1] == 0.0 and nu[0, 1] > 0 and not np.any(nu[:, 0] == nu[:, 1])
    vectors = G.root_vectors(pb, lam, mu, nu, families=fam, error_model=pr.error_model)
    ctx = capi.Context(pb)
    try:
        got = _every_rule_and_root_mass(ctx, pb, pr, fam, lam, mu, nu, vectors)
    finally:
        ctx.close()
    assert np.isfinite(got).all()


@pytest.mark.gpu
def test_a_saturated_key_keeps_its_row_zero(capi):
    """lambda t and mu t of bd_lm_ref.SATURATED on the tree's longest branch: that branch's rows s >= 1 are 0 and its row 0 is the
    negative binomial law, so a family is possible only through an absent parent -- and with a gain rate it is."""
    n = 33
    M, Rr = sizes(n)
    pb = _explicit_problem(TREE3, families(n), M, Rr)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    sat = np.array(R.SATURATED[:2]) * R.SATURATED[2] / 61.337
    assert R.rates(sat[0], sat[1], 61.337)[2] and not R.rates(sat[0], sat[1], 23.904)[2]
    lam, mu, nu = np.full((4, 1), sat[0]), np.full((4, 1), sat[1]), np.full((4, 1), 0.004)
    vectors = G.root_vectors(pb, lam, mu, nu)
    ctx = capi.Context(pb)
    try:
        got = _every_rule_and_root_mass(ctx, pb, pr, np.arange(4), lam, mu, nu, vectors)
        ctx.set_root_rule("sum")
        none = ctx.score_per_family_gain(pr, np.arange(4), lam, mu, 0 * nu, 0.2)
        twin = ctx.score_per_family_lm(pr, np.arange(4), lam, mu)
        ctx.set_root_rule("max")
    finally:
        ctx.close()
    assert np.isfinite(got).all()
    assert np.all(twin == -np.inf) and np.all(none == -np.inf)         # without gain the (A, B) branch needs an absent root and A = B = C = 0


def _no_gain_case(capi, n, error):
    M, Rr = sizes(n)
    rows = families(n)
    species = sorted(rows[0])
    table = np.array([[r[s] for s in species] for r in rows], dtype=np.int32)
    pb = P.build_problem(P.parse_newick(TREE3), species, ["f%d" % i for i in range(4)], table, root_filter=False, max_family_size=M,
                         max_root_family_size=Rr, n_deviations=3 if error else 0)
    em = None
    if error:
        em = np.tile(np.array([0.05, 0.9, 0.05]), (M + 1, 1))
        em[0] = [0.0, 0.95, 0.05]
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr), error_model=em)
    fam, zero = np.arange(4), np.zeros((4, 1))
    ctx = capi.Context(pb)
    try:
        for rule in RULES:
            ctx.set_root_rule(rule)
            two = ctx.score_per_family_lm(pr, fam, LAM, MU)
            one = ctx.score_per_family(pr, fam, LAM)
            assert np.isfinite(two).all() and np.isfinite(one).all()
            assert np.array_equal(ctx.score_per_family_gain(pr, fam, LAM, MU, zero, 0.0), two), rule
            assert np.array_equal(ctx.score_per_family_gain(pr, fam, LAM, LAM, zero, 0.0), one), rule
            assert np.array_equal(ctx.score_per_family_gain(pr, fam, LAM, None, zero, 0.0), one), rule
            assert not np.any(ctx.score_per_family_gain(pr, fam, LAM, MU, NU, 0.0) == two)       # the gain rate is read
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,error", [(n, False) for n in EVERY_WIDTH] + [(n, True) for n in (128, 641, 2048)])
def test_no_gain_is_the_two_rate_entry_bit_for_bit(capi, n, error):
    assert sorted({width(m) for m in EVERY_WIDTH}) == WIDTHS
    _no_gain_case(capi, n, error)


@pytest.mark.gpu
@pytest.mark.parametrize("error", [False, True])
def test_the_absent_profile_is_an_all_zero_family(capi, error):
    """CAFE_FAMILY_ABSENT on a table without an all-zero family == the same call on a table that holds one."""
    n = 129
    M, Rr = sizes(n)
    species = ["A", "B", "C"]
    rows = families(n)
    assert not any(all(c == 0 for c in r.values()) for r in rows)
    em = None
    if error:
        em = np.tile(np.array([0.05, 0.9, 0.05]), (M + 1, 1))
        em[0] = [0.0, 0.95, 0.05]
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_poisson(Rr, 3.0), error_model=em)
    got = []
    for with_zero in (False, True):
        table = np.array([[r[s] for s in species] for r in rows + ([dict.fromkeys(species, 0)] if with_zero else [])], dtype=np.int32)
        pb = P.build_problem(P.parse_newick(TREE3), species, ["f%d" % i for i in range(len(table))], table, root_filter=False,
                             max_family_size=M, max_root_family_size=Rr, n_deviations=3 if error else 0)
        assert pb.n_families == len(table)
        ctx = capi.Context(pb)
        try:
            vals = []
            for rule in RULES:
                ctx.set_root_rule(rule)
                fam = np.array([0, 4 if with_zero else capi.CAFE_FAMILY_ABSENT, 2, 4 if with_zero else capi.CAFE_FAMILY_ABSENT])
                vals.append(ctx.score_per_family_gain(pr, fam, LAM, MU, NU, 0.3))
            got.append(np.concatenate(vals))
        finally:
            ctx.close()
    assert np.isfinite(got[0]).all()
    assert np.array_equal(got[0], got[1])


@pytest.mark.gpu
def test_the_total_mass_of_all_profiles(capi):
    """Two taxa, order 24, every one of the 24^2 profiles a family: under the sum rule the values add up to 1 minus the mass
    that leaves the truncation, which the numpy reference computes from the row sums of its matrices.  Zeros left in row 0
    would miss it."""
    M = Rr = 23
    species = ["A", "B"]
    table = np.array([[a, b] for a in range(M + 1) for b in range(M + 1)], dtype=np.int32)
    pb = P.build_problem(P.parse_newick("(A:20,B:35);"), species, ["f%d" % i for i in range(len(table))], table, root_filter=False,
                         max_family_size=M, max_root_family_size=Rr)
    assert pb.matrix_size == 24 and pb.n_families == 576
    prior = P.prior_poisson(Rr, 6.0)
    pr = P.Params(lambdas=np.ones(1), prior=prior)
    lam, mu, nu, absent = 0.02, 0.015, 0.05, 0.3
    mats = G.matrices(pb, [lam], [mu], [nu])
    mass = np.concatenate([[absent], (1 - absent) * prior.astype(np.float64)])
    kept = float(np.sum(mass * np.prod([m[:Rr + 1, :M + 1].sum(axis=1) for m in mats if m is not None], axis=0)))
    assert 0.5 < kept < 1.0 - 1e-6
    ctx = capi.Context(pb)
    try:
        ctx.set_root_rule("sum")
        F = pb.n_families
        got = ctx.score_per_family_gain(pr, np.arange(F), np.full(F, lam), np.full(F, mu), np.full(F, nu), absent)
    finally:
        ctx.close()
    total = float(np.exp(got).sum())
    print("sum of exp(lnL) %.15f, 1 - truncated mass %.15f, difference %.3e" % (total, kept, total - kept))
    assert abs(total - kept) <= 1e-10
    stays_absent = absent * np.prod([m[0, 0] for m in mats if m is not None])
    assert got[0] > np.log(stays_absent)                     # the all-zero profile: an absent root that gains nothing, and more


@pytest.mark.gpu
def test_the_batch_cut_changes_no_value(capi, monkeypatch):
    """Order 1281 (E = 24): one family per batch and the automatic batch give the same bits, the absent profile included."""
    n = 1281
    M, Rr = sizes(n)
    pb = _explicit_problem(TREE3, families(n) + [{"A": 7, "B": 0, "C": 3}, {"A": 120, "B": 111, "C": 130}, {"A": 1, "B": 1, "C": 1}], M, Rr)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    fam = np.array([6, 0, -1, 1, 2, 3, 4, 5, 1, -1, 6])
    pick = np.arange(len(fam)) % 4
    results = []
    for cap in (1, 0):
        monkeypatch.setenv("CAFE_PER_FAMILY_BATCH", str(cap))
        ctx = capi.Context(pb)
        try:
            results.append(ctx.score_per_family_gain(pr, fam, LAM[pick], MU[pick], NU[pick], 0.2))
        finally:
            ctx.close()
    assert np.isfinite(results[0]).all()
    assert np.array_equal(results[0], results[1])


@pytest.mark.gpu
def test_values_the_host_decides(capi):
    pb = R.problem(41)
    pr = R.params(pb, "base")
    F = pb.n_families
    fam = np.arange(F)
    lam, mu, nu = np.tile(R.LAMBDAS, (F, 1)), np.tile(R.MUS, (F, 1)), np.tile([0.003, 0.001], (F, 1))
    ctx = capi.Context(pb)
    try:
        valid = ctx.score_per_family_gain(pr, fam, lam, mu, nu, 0.1)
        bad_mu, nan_lam = mu.copy(), lam.copy()
        bad_mu[1, 1] = -1e-9                                 # a negative mu: -inf
        nan_lam[2, 0] = np.nan                               # several lambdas: a NaN passes the rule and gives NaN
        got = ctx.score_per_family_gain(pr, fam, nan_lam, bad_mu, nu, 0.1)
        ctx.set_death_rates(3 * R.MUS)                       # the context's own death rates are not read
        assert np.array_equal(ctx.score_per_family_gain(pr, fam, lam, mu, nu, 0.1), valid)
        ctx.set_death_rates(None)
        for bad in (-1e-9, np.nan):
            worse = nu.copy()
            worse[5, 1] = bad
            with pytest.raises(capi.CafeError, match="code 1"):
                ctx.score_per_family_gain(pr, fam, lam, mu, worse, 0.1)
        for absent in (-0.01, 1.01, np.nan):
            with pytest.raises(capi.CafeError, match="code 1"):
                ctx.score_per_family_gain(pr, fam, lam, mu, nu, absent)
        with pytest.raises(capi.CafeError, match="code 1"):  # only -1 stands for the absent profile
            ctx.score_per_family_gain(pr, [0, -2], lam[:2], mu[:2], nu[:2], 0.1)
        with pytest.raises(capi.CafeError, match="code 1"):  # base model only
            ctx.score_per_family_gain(R.params(pb, "gamma"), [0], lam[:1], mu[:1], nu[:1], 0.1)
        everything_absent = ctx.score_per_family_gain(pr, [-1], lam[:1], mu[:1], 0 * nu[:1], 1.0)
    finally:
        ctx.close()
    keep = np.array([0, 3, 4, 5, 6, 7])
    assert np.isfinite(valid).all() and np.array_equal(got[keep], valid[keep])
    assert got[1] == -np.inf and np.isnan(got[2])
    assert everything_absent[0] == 0.0                       # root absent for sure, no gain: the all-zero profile has probability 1
