"""cafe_score_gain (gain_dense.hip): the gain model under one shared rate set on the dense prune -- every matrix built once and
stored k-major, a product kernel and an fp64 MFMA GEMM per tree level, one panel column per list entry.

Reference: the numpy prune of tests/gain_ref.py (root_vectors + reduce_root; tests/test_gain_model.py pins it to the matrix
exponential).  Tolerance: the per-family one, test_lambda_per_family._close at REL = 1e-10, infinities matched exactly -- a GEMM
sums in another order than the per-family kernel, so its bits are not asked for.  What must hold bit for bit is that a value
depends on the family and the rates alone: not on its place in the list, not on the batch cut."""
import numpy as np
import pytest

import bd_lm_ref as R
import gain_ref as G
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_gain_gpu import ABSENT, RULES, _six_taxon
from test_gain_model import six_taxon_rates
from test_lambda_per_family import _close
from test_per_family_shapes import ORDERS, TREE3, families, sizes

# the ladder of the builder's widths, and the GEMM's K-step (16) and row-tile (64) edges
DENSE_ORDERS = sorted(set(ORDERS) | {15, 16, 17, 63, 64, 65, 128, 129})


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _tiled(rates, n):
    return [np.tile(np.atleast_1d(x), (n, 1)) for x in rates]


def _against_the_numpy_prune(ctx, pb, pr, fam, rates, per_family=False):
    """score_gain under both root rules and both root masses against one set of root vectors; returns the last values"""
    vectors = G.root_vectors(pb, *_tiled(rates, len(fam)), families=fam, error_model=pr.error_model)
    got = None
    try:
        for rule in RULES:
            ctx.set_root_rule(rule)
            for absent in ABSENT:
                got = ctx.score_gain(pr, fam, *rates, absent)
                print("%s rule, root_absent %g: " % (rule, absent), end="")
                _close(got, np.array([G.reduce_root(L, pr.prior, absent, rule) for L in vectors]))
                if per_family:
                    _close(got, ctx.score_per_family_gain(pr, fam, *_tiled(rates, len(fam)), absent))
    finally:
        ctx.set_root_rule("max")
    return got


def _tree3(n):
    M, Rr = sizes(n)
    pb = _explicit_problem(TREE3, families(n), M, Rr)
    assert pb.matrix_size == n and pb.n_families == 4
    return pb, P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))


@pytest.mark.gpu
@pytest.mark.parametrize("n", DENSE_ORDERS)
def test_every_order_against_the_numpy_prune(capi, n):
    pb, pr = _tree3(n)
    fam = np.array([0, 1, 2, 3, capi.CAFE_FAMILY_ABSENT])
    ctx = capi.Context(pb)
    try:
        for rates in (G.RATES3[1], G.RATES3[3]):             # lambda < mu, lambda > mu
            got = _against_the_numpy_prune(ctx, pb, pr, fam, [rates[:1], rates[1:2], rates[2:]])
            assert np.isfinite(got).all()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order,error,missing", [(41, False, False), (300, False, False), (41, True, False), (41, False, True)])
def test_the_six_taxon_tree(capi, order, error, missing):
    """A trifurcation, a leaf under the root, two lambda indices with different nu; rate set 0 has lambda_2 = 0 < nu_2, the
    Poisson row 0.  Against the numpy prune and against the per-family entry with the rates tiled."""
    pb = _six_taxon(order, error, missing)
    pr = R.params(pb, "error" if error else "base")
    lam, mu, nu = six_taxon_rates(pb)
    assert lam[0, 1] == 0.0 and nu[0, 1] > 0 and lam[1, 1] > 0
    fam = np.concatenate([np.arange(pb.n_families), [capi.CAFE_FAMILY_ABSENT]])
    ctx = capi.Context(pb)
    try:
        for i in (0, 1):
            _against_the_numpy_prune(ctx, pb, pr, fam, [lam[i], mu[i], nu[i]], per_family=True)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_column_tile_and_batch_edges_change_no_bit(capi, monkeypatch):
    pb, pr = _tree3(65)
    rates = (G.RATES3[2, :1], G.RATES3[2, 1:2], G.RATES3[2, 2:])
    pool = np.array([0, 1, 2, 3, capi.CAFE_FAMILY_ABSENT])
    lists = {n: pool[np.arange(n) % 5] for n in (1, 127, 128, 129, 257)}
    ctx = capi.Context(pb)
    try:
        alone = {f: ctx.score_gain(pr, [f], *rates, 0.2)[0] for f in pool}
        assert np.isfinite(list(alone.values())).all() and len(set(alone.values())) == 5
        for n, fam in lists.items():
            assert np.array_equal(ctx.score_gain(pr, fam, *rates, 0.2), [alone[f] for f in fam]), n
    finally:
        ctx.close()
    monkeypatch.setenv("CAFE_PER_FAMILY_BATCH", "1")
    ctx = capi.Context(pb)
    try:
        assert np.array_equal(ctx.score_gain(pr, lists[257], *rates, 0.2), [alone[f] for f in lists[257]])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_saturated_key_keeps_its_row_zero(capi):
    """test_gain_gpu's rates at n = 33: the (A, B) branch's rows s >= 1 are 0, its row 0 the negative binomial law"""
    pb, pr = _tree3(33)
    sat = np.array(R.SATURATED[:2]) * R.SATURATED[2] / 61.337
    assert R.rates(sat[0], sat[1], 61.337)[2] and not R.rates(sat[0], sat[1], 23.904)[2]
    ctx = capi.Context(pb)
    try:
        got = _against_the_numpy_prune(ctx, pb, pr, np.arange(4), [sat[:1], sat[1:], np.array([0.004])])
        ctx.set_root_rule("sum")
        none = ctx.score_gain(pr, np.arange(4), sat[:1], sat[1:], [0.0], 0.2)
    finally:
        ctx.close()
    assert np.isfinite(got).all() and np.all(none == -np.inf)


@pytest.mark.gpu
def test_no_gain_is_the_two_rate_entry_to_rounding(capi):
    pb, pr = _tree3(129)
    lam, mu = G.RATES3[:, 0], G.RATES3[:, 1]
    ctx = capi.Context(pb)
    try:
        for rule in RULES:
            ctx.set_root_rule(rule)
            for i in range(4):
                got = ctx.score_gain(pr, np.arange(4), lam[i:i + 1], mu[i:i + 1], [0.0], 0.0)
                _close(got, ctx.score_per_family_lm(pr, np.arange(4), np.full(4, lam[i]), np.full(4, mu[i])))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_values_the_host_decides(capi):
    pb = R.problem(41)
    pr = R.params(pb, "base")
    fam = np.arange(pb.n_families)
    lam, mu, nu = R.LAMBDAS, R.MUS, np.array([0.003, 0.001])
    ctx = capi.Context(pb)
    try:
        before = ctx.score(pr)
        assert np.isfinite(ctx.score_gain(pr, fam, lam, mu, nu, 0.1)).all()
        assert ctx.score(pr) == before                       # a later cafe_score returns what it returned before
        assert np.all(ctx.score_gain(pr, fam, lam, [mu[0], -1e-9], nu, 0.1) == -np.inf)
        assert np.isnan(ctx.score_gain(pr, fam, [np.nan, lam[1]], mu, nu, 0.1)).all()
        for bad in ([0.003, -1e-9], [np.nan, 0.001]):
            with pytest.raises(capi.CafeError, match="code 1: cafe_score_gain: gain rate"):
                ctx.score_gain(pr, fam, lam, mu, bad, 0.1)
        for absent in (-0.01, 1.01, np.nan):
            with pytest.raises(capi.CafeError, match="code 1: cafe_score_gain: root_absent"):
                ctx.score_gain(pr, fam, lam, mu, nu, absent)
        with pytest.raises(capi.CafeError, match="code 1: cafe_score_gain: family index -2"):
            ctx.score_gain(pr, [0, -2], lam, mu, nu, 0.1)
        with pytest.raises(capi.CafeError, match="code 1: cafe_score_gain: base model only"):
            ctx.score_gain(R.params(pb, "gamma"), [0], lam, mu, nu, 0.1)
        assert ctx.score_gain(pr, [-1], lam, mu, 0 * nu, 1.0)[0] == 0.0      # root absent for sure, no gain: probability 1
        ctx.comm_attach(capi.comm_unique_id(), 1, 0)         # a communicator of one rank
        with pytest.raises(capi.CafeError, match="code 4: cafe_score_gain: not valid on a context with a communicator attached"):
            ctx.score_gain(pr, fam, lam, mu, nu, 0.1)
        ctx.comm_detach()
    finally:
        ctx.close()
