"""cafe_gain_posterior_dense (gain_dense.hip) against the numpy down pass of tests/gain_posterior_ref.py with the rate set tiled.
Tolerance: test_gain_posterior_gpu._close -- relative 1e-10, references below 1e-290 compared absolutely against 1e-290.  lnl is
compared with score_gain's under the sum rule by ==, and a value across places in the list and batch cuts by ==."""
import numpy as np
import pytest

import bd_lm_ref as R
import gain_posterior_ref as GP
import gain_ref as G
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_gain_dense_gpu import _tiled
from test_gain_gpu import _six_taxon
from test_gain_model import six_taxon_rates
from test_gain_posterior_gpu import ABSENT, _close, capi  # noqa: F401 (the fixture)
from test_gain_posterior_model import three_taxon
from test_per_family_shapes import TREE3, sizes

PAIRS = [(2, 2), (12, 14), (15, 16), (16, 15), (63, 64), (64, 63), (64, 80), (128, 127), (240, 299), (512, 640)]


def _check(ctx, pb, pr, fam, rates, absent, missing_leaves=(), cache=None):
    """Every output against the reference; lnl == score_gain's; the root rule stays `max`; the posteriors sum to 1"""
    ctx.set_root_rule("max")
    got = ctx.gain_posterior_dense(pr, fam, *rates, absent, want_posterior=True)
    assert ctx.root_rule() == "max"
    want = GP.table(pb, fam, *_tiled(rates, len(fam)), pr.prior, absent, pr.error_model, cache=cache)
    print("root_absent %g: " % absent, end="")
    for key in ("lnl",) + GP.KEYS:
        _close(got[key], want[key], key)
    print()
    ctx.set_root_rule("sum")
    assert np.array_equal(got["lnl"], ctx.score_gain(pr, fam, *rates, absent))
    ctx.set_root_rule("max")
    assert np.isfinite(got["lnl"]).all()
    total = got["posterior"].sum(axis=2)
    keep = np.ones(total.shape, dtype=bool)
    for f, v in missing_leaves:
        keep[f, v] = False
    assert np.max(np.abs(total[keep] - 1.0)) <= 1e-12
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("M,Rr", PAIRS)
def test_every_tile_edge_against_the_numpy_down_pass(capi, M, Rr):
    """At root_absent 0.2 and the first seven pairs the reference must be informative: >= 3 families each with a p_gain / p_loss
    in [0.05, 0.95] on some branch (with root_absent 0 only 2 are).  M + 1 and R + 1 stand either side of 16, 64 and 128."""
    n = max(M, Rr) + 1
    pb = _explicit_problem(TREE3, GP.patchy_families(n, M), M, Rr)
    assert pb.matrix_size == n and pb.n_families == 6
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    root = int(np.where(pb.parent < 0)[0][0])
    ctx = capi.Context(pb)
    try:
        for rates in (G.RATES3[1], G.RATES3[3]):             # lambda < mu, lambda > mu
            cache = {}
            for absent in ABSENT:
                got, want = _check(ctx, pb, pr, np.arange(6), [rates[:1], rates[1:2], rates[2:]], absent, cache=cache)
                assert np.isnan(got["p_gain"][:, root]).all() and np.isnan(got["p_loss"][:, root]).all()
                if absent > 0 and (M, Rr) in PAIRS[:7]:
                    for key in ("p_gain", "p_loss"):
                        with np.errstate(invalid="ignore"):
                            assert ((want[key] >= 0.05) & (want[key] <= 0.95)).any(axis=1).sum() >= 3, key
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order,error,missing", [(41, False, False), (300, False, False), (41, True, False), (41, False, True)])
def test_the_six_taxon_tree(capi, order, error, missing):
    """Depth >= 2 (the contraction is M + 1), a trifurcation, a leaf under the root; also against the per-family entry"""
    pb = _six_taxon(order, error, missing)
    pr = R.params(pb, "error" if error else "base")
    lam, mu, nu = six_taxon_rates(pb)
    fam = np.concatenate([np.arange(pb.n_families), [capi.CAFE_FAMILY_ABSENT]])
    leaf_of = {int(t): v for v, t in enumerate(pb.leaf_taxon) if t >= 0}
    missing_leaves = [(f, leaf_of[t]) for f in range(pb.n_families) for t in range(pb.n_taxa) if pb.counts[f, t] < 0]
    assert bool(missing_leaves) == missing
    ctx = capi.Context(pb)
    try:
        for i in (0, 1):
            rates = [lam[i], mu[i], nu[i]]
            got, _ = _check(ctx, pb, pr, fam, rates, 0.2, missing_leaves)
            per_family = ctx.gain_posterior(pr, fam, *_tiled(rates, len(fam)), 0.2, want_posterior=True)
            for key in ("lnl",) + GP.KEYS:
                _close(got[key], per_family[key], key)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_place_and_batch_change_no_bit(capi, monkeypatch):
    pb = three_taxon(65)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(sizes(65)[1]))
    rates = (G.RATES3[2, :1], G.RATES3[2, 1:2], G.RATES3[2, 2:])
    pool = np.array([0, 1, 2, 3, 4, 5, capi.CAFE_FAMILY_ABSENT])
    lists = {n: pool[np.arange(n) % 7] for n in (1, 127, 128, 129, 257)}

    def same(got, fam, alone):
        for key in got:
            assert np.array_equal(got[key], np.array([alone[f][key][0] for f in fam]), equal_nan=True), (len(fam), key)
    ctx = capi.Context(pb)
    try:
        alone = {f: ctx.gain_posterior_dense(pr, [f], *rates, 0.2, want_posterior=True) for f in pool}
        assert all(np.isfinite(a["lnl"]).all() for a in alone.values()) and len({a["lnl"][0] for a in alone.values()}) == 7
        for fam in lists.values():
            same(ctx.gain_posterior_dense(pr, fam, *rates, 0.2, want_posterior=True), fam, alone)
    finally:
        ctx.close()
    monkeypatch.setenv("CAFE_PER_FAMILY_BATCH", "1")
    ctx = capi.Context(pb)
    try:
        same(ctx.gain_posterior_dense(pr, lists[257], *rates, 0.2, want_posterior=True), lists[257], alone)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_what_the_host_and_the_zeros_decide(capi):
    def nothing(got, lnl):
        assert np.array_equal(got["lnl"], np.full(len(got["lnl"]), lnl), equal_nan=True)
        for key in GP.KEYS:
            assert np.isnan(got[key]).all(), key
    n = 33                                                   # test_gain_dense_gpu's saturated key
    pb = three_taxon(n)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(sizes(n)[1]))
    sat = np.array(R.SATURATED[:2]) * R.SATURATED[2] / 61.337
    assert R.rates(sat[0], sat[1], 61.337)[2] and not R.rates(sat[0], sat[1], 23.904)[2]
    ctx = capi.Context(pb)
    try:
        _check(ctx, pb, pr, np.arange(6), [sat[:1], sat[1:], np.array([0.004])], 0.2)
        nothing(ctx.gain_posterior_dense(pr, np.arange(6), sat[:1], sat[1:], [0.0], 0.0, want_posterior=True), -np.inf)
    finally:
        ctx.close()
    pb = three_taxon(129)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(sizes(129)[1]))
    root = int(np.where(pb.parent < 0)[0][0])
    ctx = capi.Context(pb)
    try:
        got = ctx.gain_posterior_dense(pr, np.arange(6), G.RATES3[1, :1], G.RATES3[1, 1:2], [0.0], 0.0)
    finally:
        ctx.close()
    finite = np.isfinite(got["lnl"])
    assert finite.sum() >= 1 and np.all(got["p_gain"][finite][:, np.arange(pb.n_nodes) != root] == 0.0)
    assert np.isnan(got["p_absent"][~finite]).all() and np.all(got["lnl"][~finite] == -np.inf)
    pb = R.problem(41)
    pr = R.params(pb, "base")
    fam = np.arange(pb.n_families)
    lam, mu, nu = R.LAMBDAS, R.MUS, np.array([0.003, 0.001])
    ctx = capi.Context(pb)
    try:
        before = ctx.score(pr)
        assert np.isfinite(ctx.gain_posterior_dense(pr, fam, lam, mu, nu, 0.1)["lnl"]).all()
        assert ctx.score(pr) == before
        nothing(ctx.gain_posterior_dense(pr, fam, lam, [mu[0], -1e-9], nu, 0.1, want_posterior=True), -np.inf)
        nothing(ctx.gain_posterior_dense(pr, fam, [np.nan, lam[1]], mu, nu, 0.1, want_posterior=True), np.nan)
        with pytest.raises(capi.CafeError, match="code 1: cafe_gain_posterior_dense: gain rate"):
            ctx.gain_posterior_dense(pr, fam, lam, mu, [0.003, -1e-9], 0.1)
        with pytest.raises(capi.CafeError, match="code 1: cafe_gain_posterior_dense: root_absent"):
            ctx.gain_posterior_dense(pr, fam, lam, mu, nu, 1.01)
        with pytest.raises(capi.CafeError, match="code 1: cafe_gain_posterior_dense: family index -2"):
            ctx.gain_posterior_dense(pr, [0, -2], lam, mu, nu, 0.1)
        with pytest.raises(capi.CafeError, match="code 1: cafe_gain_posterior_dense: base model only"):
            ctx.gain_posterior_dense(R.params(pb, "gamma"), [0], lam, mu, nu, 0.1)
        ctx.comm_attach(capi.comm_unique_id(), 1, 0)         # a communicator of one rank
        with pytest.raises(capi.CafeError, match="code 4: cafe_gain_posterior_dense: not valid on a context with a communicator attached"):
            ctx.gain_posterior_dense(pr, fam, lam, mu, nu, 0.1)
        ctx.comm_detach()
    finally:
        ctx.close()
