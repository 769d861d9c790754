"""cafe_gain_posterior (family_gain_posterior.hip, family_gain_down_kernel.h): posterior absence, origin and loss on every
branch under the gain model.

Reference: the numpy down pass of tests/gain_posterior_ref.py (tests/test_gain_posterior_model.py pins it to the enumeration
of every interior size assignment and shows what these tables tell apart).  Tolerance: the per-family one, relative 1e-10
(test_lambda_per_family.REL); reference values below 1e-290 are compared absolutely against 1e-290, because denormals cannot
hold ten digits.  lnl is compared with score_per_family_gain's under the sum rule by ==.  A reference is computed once per
table and root mass; the matrices are shared by the root masses."""
import numpy as np
import pytest

import bd_lm_ref as R
import gain_posterior_ref as GP
import gain_ref as G
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_gain_gpu import _six_taxon
from test_gain_model import six_taxon_rates
from test_gain_posterior_model import rates3, three_taxon
from test_lambda_per_family import REL
from test_per_family_shapes import ORDERS, TREE3, sizes, width

ABSENT = (0.0, 0.2)
FLOOR = 1e-290


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got)), what
    rel = np.max(np.abs(got[~nan] - want[~nan]) / np.maximum(np.abs(want[~nan]), FLOOR))
    print("%s %.3e " % (what, rel), end="")
    assert rel <= REL, (what, rel)


def _check(ctx, pb, pr, fam, lam, mu, nu, missing_leaves=(), masses=ABSENT):
    """Every output at both root masses against the reference; lnl against the score entry bit for bit; the posteriors sum to
    1; the root rule is what it was.  Returns the results of the last root mass."""
    cache, got = {}, None
    for rule in ("max", "sum"):
        ctx.set_root_rule(rule)
        for absent in masses if rule == "max" else masses[-1:]:
            got = ctx.gain_posterior(pr, fam, lam, mu, nu, absent, want_posterior=True)
            assert ctx.root_rule() == rule
            want = GP.table(pb, fam, lam, mu, nu, pr.prior, absent, pr.error_model, cache=cache)
            print("root_absent %g, %s rule set: " % (absent, rule), end="")
            for key in ("lnl",) + GP.KEYS:
                _close(got[key], want[key], key)
            print()
            ctx.set_root_rule("sum")
            assert np.array_equal(got["lnl"], ctx.score_per_family_gain(pr, fam, lam, mu, nu, absent))
            ctx.set_root_rule(rule)
            assert np.isfinite(got["lnl"]).all()
            total = got["posterior"].sum(axis=2)
            keep = np.ones(total.shape, dtype=bool)
            for f, v in missing_leaves:
                keep[f, v] = False
            assert np.max(np.abs(total[keep] - 1.0)) <= 1e-12
            no_posterior = ctx.gain_posterior(pr, fam, lam, mu, nu, absent)
            assert "posterior" not in no_posterior
            for key in no_posterior:
                assert np.array_equal(no_posterior[key], got[key], equal_nan=True), key
    ctx.set_root_rule("max")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", ORDERS)
def test_every_width_against_the_numpy_down_pass(capi, n):
    """The patchy profiles and the family near n / 4, each under its own (lambda, mu, nu), either side of every switch of the
    width ladder."""
    pb = three_taxon(n)
    assert pb.matrix_size == n and pb.n_families == 6
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(sizes(n)[1]))
    lam, mu, nu = rates3(pb)
    ctx = capi.Context(pb)
    try:
        got = _check(ctx, pb, pr, np.arange(6), lam, mu, nu)
    finally:
        ctx.close()
    root = int(np.where(pb.parent < 0)[0][0])
    assert np.isnan(got["p_gain"][:, root]).all() and np.isnan(got["p_loss"][:, root]).all()
    print("n %d E %d: largest p_gain %s" % (n, width(n), np.nanmax(got["p_gain"], axis=1)))


@pytest.mark.gpu
@pytest.mark.parametrize("order,error,missing", [(41, False, False), (300, False, False), (41, True, False), (41, False, True)])
def test_the_six_taxon_tree(capi, order, error, missing):
    """test_gain_gpu's settings: a trifurcation, a leaf under the root, two lambda indices with different nu, the Poisson row 0,
    the all-zero profile as a listed family; with a 3-tap error model; with missing cells."""
    pb = _six_taxon(order, error, missing)
    pr = R.params(pb, "error" if error else "base")
    lam, mu, nu = six_taxon_rates(pb)
    fam = np.concatenate([np.arange(pb.n_families), [capi.CAFE_FAMILY_ABSENT]])
    lam, mu, nu = (np.concatenate([x, x[2:3]]) for x in (lam, mu, nu))
    leaf_of = {int(t): v for v, t in enumerate(pb.leaf_taxon) if t >= 0}
    missing_leaves = [(f, leaf_of[t]) for f in range(pb.n_families) for t in range(pb.n_taxa) if pb.counts[f, t] < 0]
    assert bool(missing_leaves) == missing
    ctx = capi.Context(pb)
    try:
        _check(ctx, pb, pr, fam, lam, mu, nu, missing_leaves)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_saturated_key(capi):
    """test_gain_gpu's saturated rates on the tree's longest branch: the down kernel runs row 0 of that branch alone, so the
    node below it hears of its parent only through an absent parent -- every family needs root_absent > 0 to be possible.  With
    root_absent = 0, and without a gain rate, lnl is -inf from the device: NaN in every other output."""
    n = 33
    pb = three_taxon(n)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(sizes(n)[1]))
    sat = np.array(R.SATURATED[:2]) * R.SATURATED[2] / 61.337
    assert R.rates(sat[0], sat[1], 61.337)[2] and not R.rates(sat[0], sat[1], 23.904)[2]
    lam, mu, nu = np.full((6, 1), sat[0]), np.full((6, 1), sat[1]), np.full((6, 1), 0.004)
    ctx = capi.Context(pb)
    try:
        _check(ctx, pb, pr, np.arange(6), lam, mu, nu, masses=ABSENT[1:])
        impossible = [ctx.gain_posterior(pr, np.arange(6), lam, mu, rate, 0.0, want_posterior=True) for rate in (nu, 0 * nu)]
        ctx.set_root_rule("sum")
        assert np.array_equal(impossible[0]["lnl"], ctx.score_per_family_gain(pr, np.arange(6), lam, mu, nu, 0.0))
        ctx.set_root_rule("max")
    finally:
        ctx.close()
    for none in impossible:
        assert np.all(none["lnl"] == -np.inf)
        for key in GP.KEYS:
            assert np.isnan(none[key]).all(), key


@pytest.mark.gpu
def test_without_a_gain_rate_nothing_originates(capi):
    n = 129
    pb = three_taxon(n)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(sizes(n)[1]))
    lam, mu, nu = rates3(pb)
    root = int(np.where(pb.parent < 0)[0][0])
    ctx = capi.Context(pb)
    try:
        got = ctx.gain_posterior(pr, np.arange(6), lam, mu, 0 * nu, 0.0)
    finally:
        ctx.close()
    finite = np.isfinite(got["lnl"])
    assert finite.sum() >= 4
    branches = np.arange(pb.n_nodes) != root
    assert np.all(got["p_gain"][finite][:, branches] == 0.0)
    assert np.nanmax(got["p_loss"]) > 0.05                   # (what was there can still be lost)
    assert np.isnan(got["p_absent"][~finite]).all() and np.all(got["lnl"][~finite] == -np.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("error", [False, True])
def test_the_absent_profile_is_an_all_zero_family(capi, error):
    """CAFE_FAMILY_ABSENT on a table without an all-zero family == the same call on a table that holds one."""
    n = 129
    M, Rr = sizes(n)
    rows = GP.patchy_families(n, M)
    species = ["A", "B", "C"]
    em = None
    if error:
        em = np.tile(np.array([0.05, 0.9, 0.05]), (M + 1, 1))
        em[0] = [0.0, 0.95, 0.05]
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_poisson(Rr, 3.0), error_model=em)
    pick = np.arange(4)
    got = []
    for with_zero in (False, True):
        table = np.array([[r[s] for s in species] for r in rows + ([dict.fromkeys(species, 0)] if with_zero else [])], dtype=np.int32)
        pb = P.build_problem(P.parse_newick(TREE3), species, ["f%d" % i for i in range(len(table))], table, root_filter=False,
                             max_family_size=M, max_root_family_size=Rr, n_deviations=3 if error else 0)
        zero = 6 if with_zero else capi.CAFE_FAMILY_ABSENT
        ctx = capi.Context(pb)
        try:
            got.append(ctx.gain_posterior(pr, [0, zero, 5, zero], G.RATES3[pick, :1], G.RATES3[pick, 1:2], G.RATES3[pick, 2:], 0.3, want_posterior=True))
        finally:
            ctx.close()
    assert np.isfinite(got[0]["lnl"]).all() and got[0]["p_absent"][1].max() > 0.5
    for key in got[0]:
        assert np.array_equal(got[0][key], got[1][key], equal_nan=True), key


@pytest.mark.gpu
def test_the_batch_cut_changes_no_value(capi, monkeypatch):
    """Order 1281 (E = 24): one family per batch and the automatic batch give the same bits, the absent profile included."""
    n = 1281
    pb = three_taxon(n)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(sizes(n)[1]))
    fam = np.array([5, 0, -1, 1, 2, 3, 4, 5, 1, -1])
    pick = np.arange(len(fam)) % 4
    results = []
    for cap in (1, 0):
        monkeypatch.setenv("CAFE_PER_FAMILY_BATCH", str(cap))
        ctx = capi.Context(pb)
        try:
            results.append(ctx.gain_posterior(pr, fam, G.RATES3[pick, :1], G.RATES3[pick, 1:2], G.RATES3[pick, 2:], 0.2, want_posterior=True))
        finally:
            ctx.close()
    assert np.isfinite(results[0]["lnl"]).all() and np.isfinite(results[0]["posterior"]).all()
    for key in results[0]:
        assert np.array_equal(results[0][key], results[1][key], equal_nan=True), key


@pytest.mark.gpu
def test_the_scorer_and_the_root_rule_are_left_alone_and_what_is_refused(capi):
    pb = R.problem(41)
    pr = R.params(pb, "base")
    F = pb.n_families
    fam = np.arange(F)
    lam, mu, nu = np.tile(R.LAMBDAS, (F, 1)), np.tile(R.MUS, (F, 1)), np.tile([0.003, 0.001], (F, 1))
    ctx = capi.Context(pb)
    try:
        for rule in ("max", "sum"):
            ctx.set_root_rule(rule)
            before = ctx.score(pr)
            valid = ctx.gain_posterior(pr, fam, lam, mu, nu, 0.1)
            assert ctx.root_rule() == rule
            assert ctx.score(pr) == before
        ctx.set_root_rule("max")
        bad_mu, nan_lam = mu.copy(), lam.copy()
        bad_mu[1, 1] = -1e-9                                 # a negative mu: -inf
        nan_lam[2, 0] = np.nan                               # several lambdas: a NaN passes the rule and gives NaN
        got = ctx.gain_posterior(pr, fam, nan_lam, bad_mu, nu, 0.1, want_posterior=True)
        keep = np.array([0, 3, 4, 5, 6, 7])
        assert got["lnl"][1] == -np.inf and np.isnan(got["lnl"][2])
        for key in GP.KEYS:
            assert np.isnan(got[key][1:3]).all(), key
            if key != "posterior":
                assert np.array_equal(got[key][keep], valid[key][keep], equal_nan=True), key
        worse = nu.copy()
        worse[5, 1] = -1e-9
        with pytest.raises(capi.CafeError, match="code 1: cafe_gain_posterior: gain rate"):
            ctx.gain_posterior(pr, fam, lam, mu, worse, 0.1)
        with pytest.raises(capi.CafeError, match="code 1: cafe_gain_posterior: base model only"):
            ctx.gain_posterior(R.params(pb, "gamma"), [0], lam[:1], mu[:1], nu[:1], 0.1)
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.gain_posterior(pr, fam, lam, mu, nu, 1.01)
        ctx.comm_attach(capi.comm_unique_id(), 1, 0)         # a communicator of one rank
        with pytest.raises(capi.CafeError, match="code 4: cafe_gain_posterior: not valid on a context with a communicator attached"):
            ctx.gain_posterior(pr, fam, lam, mu, nu, 0.1)
        ctx.comm_detach()
        again = ctx.gain_posterior(pr, fam, lam, mu, nu, 0.1)
        for key in valid:
            assert np.array_equal(again[key], valid[key], equal_nan=True), key
    finally:
        ctx.close()
