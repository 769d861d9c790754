"""cafe_gain_leaf_predictive (the fused kernel of gain_dense.hip) against the leave-one-out definition of tests/gain_predictive_ref.py.
mean and the three p's: relative 1e-10 (test_gain_posterior_gpu._close, the neighbouring dense tests' tolerance).  sd is held through the
variance, sd^2 against the reference's within 1e-10 of the reference's E[(y - x)^2]: a variance is the difference of two moments and carries
the absolute error of the larger.  lnl == score_gain's under the sum rule, and a value across places in the list and batch cuts by ==."""
from contextlib import closing

import numpy as np
import pytest

import bd_lm_ref as R
import gain_posterior_ref as GP
import gain_predictive_ref as LP
import gain_ref as G
import gain_scaled_ref as S
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_gain_gpu import _six_taxon
from test_gain_model import six_taxon_rates
from test_gain_posterior_gpu import ABSENT, _close, capi  # noqa: F401 (the fixture)
from test_gain_posterior_model import three_taxon
from test_gain_scaled_gpu import RATES, tree32, wide
from test_per_family_shapes import TREE3, sizes

PAIRS = [(2, 2), (15, 16), (16, 15), (63, 64), (64, 63), (64, 80), (128, 127), (240, 299)]


def _check(ctx, pr, fam, rates, absent, want):
    ctx.set_root_rule("max")
    got = ctx.gain_leaf_predictive(pr, fam, *rates, absent)
    ctx.set_root_rule("sum")
    assert np.array_equal(got["lnl"], ctx.score_gain(pr, fam, *rates, absent)) and np.isfinite(got["lnl"]).all()
    for key in ("mean", "p_below", "p_obs", "p_above"):
        _close(got[key], want[key], key)
    worst = np.max(np.abs(got["sd"] ** 2 - want["sd"] ** 2) / want["second"])
    print("variance %.3e" % worst)
    assert worst <= 1e-10
    total = got["p_below"] + got["p_obs"] + got["p_above"]
    assert np.nanmax(np.abs(total - 1.0)) <= 1e-12
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("M,Rr", PAIRS)
def test_every_tile_edge_against_the_leave_one_out_definition(capi, M, Rr):
    """M + 1 and R + 1 either side of 16, 64 and 128, four row tiles at (240, 299).  The table must be informative by the reference
    alone: at least 9 of the 18 cells with a smaller one-sided tail >= 0.05.  The sixth family's counts stop at those of order 65
    (16, 15, 17); pivots in the higher row tiles are the six-taxon tree's at order 300."""
    pb = _explicit_problem(TREE3, GP.patchy_families(min(max(M, Rr) + 1, 65), M), M, Rr)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    with closing(capi.Context(pb)) as ctx:
        for rates in ([[r] for r in G.RATES3[1]], [[r] for r in G.RATES3[3]]):
            cache = {}
            for absent in ABSENT:
                want = LP.table(pb, np.arange(6), rates, pr.prior, absent, cache=cache)
                tail = np.minimum(want["p_below"] + want["p_obs"], want["p_obs"] + want["p_above"])
                assert (tail >= 0.05).sum() >= 9, tail
                _check(ctx, pr, np.arange(6), rates, absent, want)


@pytest.mark.gpu
@pytest.mark.parametrize("order,error,missing", [(41, False, False), (41, True, False), (41, False, True), (300, False, False)])
def test_the_six_taxon_tree(capi, order, error, missing):
    """Depth >= 2 (the contraction is M + 1), the trifurcation, the leaf under the root, taps across a row-tile boundary; the list
    ends with the absent profile.  A missing cell has the reference's mean and sd and NaN p's (_close compares the NaN masks)."""
    pb = _six_taxon(order, error, missing)
    pr = R.params(pb, "error" if error else "base")
    fam = np.concatenate([np.arange(pb.n_families), [capi.CAFE_FAMILY_ABSENT]])
    with closing(capi.Context(pb)) as ctx:
        for i in (0, 1):
            rates = [x[i] for x in six_taxon_rates(pb)]
            got = _check(ctx, pr, fam, rates, 0.2, LP.table(pb, fam, rates, pr.prior, 0.2, pr.error_model))
            assert np.array_equal(np.isnan(got["p_obs"][:-1]), pb.counts < 0) and np.isnan(got["p_obs"]).any() == missing


@pytest.mark.gpu
def test_place_and_batch_change_no_bit(capi, monkeypatch):
    pb = three_taxon(65)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(sizes(65)[1]))
    rates = [[r] for r in G.RATES3[2]]
    pool, alone = np.array([0, 1, 2, 3, 4, 5, capi.CAFE_FAMILY_ABSENT]), None
    for n, batch in ((1, "0"), (127, "0"), (128, "0"), (129, "0"), (257, "0"), (257, "1")):
        monkeypatch.setenv("CAFE_PER_FAMILY_BATCH", batch)
        with closing(capi.Context(pb)) as ctx:
            alone = alone or [ctx.gain_leaf_predictive(pr, [f], *rates, 0.2) for f in pool]
            got = ctx.gain_leaf_predictive(pr, pool[np.arange(n) % 7], *rates, 0.2)
        for key in got:
            assert np.array_equal(got[key], np.array([alone[i % 7][key][0] for i in range(n)]), equal_nan=True), (key, n, batch)
    assert len({a["lnl"][0] for a in alone}) == 7 and all(np.isfinite(a["sd"]).all() for a in alone)


@pytest.mark.gpu
def test_the_scaled_mode_on_the_six_taxon_tree(capi):
    """Every output is a ratio inside one column: on against off at 1e-12 relative, and off again bit for bit"""
    pb = _six_taxon(41, False, True)
    pr, rates = R.params(pb, "base"), [x[1] for x in six_taxon_rates(pb)]
    with closing(capi.Context(pb)) as ctx:
        plain, scaled, again = [(ctx.set_gain_scaling(on), ctx.gain_leaf_predictive(pr, np.arange(pb.n_families), *rates, 0.2))[1] for on in (False, True, False)]
    for key in LP.KEYS:
        assert np.array_equal(plain[key], again[key], equal_nan=True) and np.array_equal(np.isnan(plain[key]), np.isnan(scaled[key]))
        assert np.nanmax(np.abs(scaled[key] - plain[key]) / np.maximum(np.abs(plain[key]), 1e-290)) <= 1e-12, key


@wide
@pytest.mark.gpu
def test_the_scaled_mode_below_the_range_of_fp64(capi):
    """tree32 (16, 8), family 0 (0 / M alternating): plain lnl -inf and NaN; scaled, the five numbers of the np.longdouble prune of
    tests/gain_scaled_ref.py, run on the 32 x 17 profiles that differ from the family in one cell"""
    pb, newick = tree32(16, 8)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(8))
    rates = [[r] for r in RATES[0]]
    with closing(capi.Context(pb)) as ctx:
        assert ctx.gain_leaf_predictive(pr, [0], *rates, 0.2)["lnl"][0] == -np.inf
        ctx.set_gain_scaling(True)
        got = ctx.gain_leaf_predictive(pr, [0], *rates, 0.2)
    rows = np.repeat(pb.counts[:1], 32 * 17, axis=0)
    rows[np.arange(32 * 17), np.repeat(np.arange(32), 17)] = np.tile(np.arange(17), 32)
    one_off = _explicit_problem(newick, [dict(zip(pb.taxa, r)) for r in rows], 16, 8)
    lnl = S.table(one_off, np.arange(32 * 17), RATES[0], pr.prior, 0.2)["lnl"].reshape(32, 17)
    want = LP.summary(np.exp(lnl - lnl.max(axis=1, keepdims=True)), pb.counts[0])
    for key in ("mean", "p_below", "p_obs", "p_above"):
        _close(got[key][0], want[key], key)
    assert np.max(np.abs(got["sd"][0] ** 2 - want["sd"] ** 2) / want["second"]) <= 1e-10


@pytest.mark.gpu
def test_what_is_refused_and_what_the_host_decides(capi):
    pb = R.problem(41)
    pr, fam, lam, mu, nu = R.params(pb, "base"), np.arange(pb.n_families), R.LAMBDAS, R.MUS, np.array([0.003, 0.001])
    with closing(capi.Context(pb)) as ctx:
        for args, why in (((pr, fam, lam, mu, [0.003, -1e-9], 0.1), "gain rate"), ((pr, fam, lam, mu, nu, 1.5), "root_absent"),
                          ((pr, [0, -2], lam, mu, nu, 0.1), "family index -2"), ((R.params(pb, "gamma"), [0], lam, mu, nu, 0.1), "base model only")):
            with pytest.raises(capi.CafeError, match="code 1: cafe_gain_leaf_predictive: " + why):
                ctx.gain_leaf_predictive(*args)
        got = ctx.gain_leaf_predictive(pr, fam, lam, [mu[0], -1e-9], nu, 0.1)
    assert np.all(got["lnl"] == -np.inf) and all(np.isnan(got[key]).all() for key in LP.KEYS)
