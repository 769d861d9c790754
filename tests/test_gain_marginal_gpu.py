"""cafe_gain_marginal_dense (gain_marginal_kernel.h) against the longdouble reference of tests/gain_marginal_ref.py at every edge of
the split GEMM's tiles; the inputs and their margins are checked on the reference alone in tests/test_gain_marginal_model.py.
Integers ==.  Doubles: relative BOUND, references below 1e-290 compared absolutely against 1e-290.  lnl == score_gain's under the sum
rule; every output == across places in the list and the batch cut."""
from contextlib import closing

import numpy as np
import pytest

import gain_marginal_ref as GM
import gain_scaled_ref as S
from cafexp_amd import problem as P
from test_gain_posterior_gpu import capi  # noqa: F401 (the fixture)
from test_gain_scaled_gpu import RATES as SCALED_RATES, tree32

RATES, SCALED = [[r] for r in GM.RATES], [[r] for r in SCALED_RATES[0]]
BOUND = 1.6e-13        # ten times the worst measured over these cases on the MI355X: 6.3e-15 plain, 1.53e-14 in the scaled mode


def _close(got, want, keys=GM.DOUBLES):
    worst = 0.0
    for key in keys:
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key].astype(np.float64))), key
        err = np.abs(got[key].astype(GM.LD) - want[key]) / np.maximum(np.abs(want[key]), 1e-290)
        worst = max(worst, float(np.nanmax(err)))
        assert worst <= BOUND, (key, worst)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", GM.CASES, ids=str)
def test_every_tile_edge_and_tree_shape_against_the_longdouble_reference(capi, case):
    """Lists of 1, 128 and 129 entries (a repeated index and CAFE_FAMILY_ABSENT among them); a workspace_limit of six panels of one column
    tile is enough to create the context and too little for a second tile of this call: it cuts the 129 into two batches"""
    pb, pr = GM.problem(*case)
    small = 6 * pb.matrix_size * 128 * 8
    pool = np.array(list(range(pb.n_families)) + [capi.CAFE_FAMILY_ABSENT])
    want = GM.table(pb, pool, GM.RATES, pr.prior, GM.ABSENT, GM.LEVEL, pr.error_model)
    got = {}
    for n, limit in ((1, 0), (128, 0), (129, 0), (129, small)):
        with closing(capi.Context(pb, workspace_limit=limit)) as ctx:
            fam = pool[(np.arange(n) + 3) % len(pool)]
            got[n, limit] = res = ctx.gain_marginal_dense(pr, fam, *RATES, GM.ABSENT, GM.LEVEL)
            ctx.set_root_rule("sum")
            assert np.array_equal(res["lnl"], ctx.score_gain(pr, fam, *RATES, GM.ABSENT))
            if (n, limit) == (129, 0):
                dense = ctx.gain_posterior_dense(pr, fam, *RATES, GM.ABSENT)
                print("mean against gain_posterior_dense's: %.3g" % _close(res, {"mean": dense["mean"].astype(GM.LD)}, ("mean",)))
        at = (np.arange(n) + 3) % len(pool)
        assert all(np.array_equal(res[key], want[key][at]) for key in GM.INTS), (n, limit)
        print("n %d limit %d worst %.3g" % (n, limit, _close(res, {k: want[k][at] for k in GM.DOUBLES})))
    for key in ("lnl",) + GM.DOUBLES + GM.INTS:                     # place and batch cut change no bit
        for (n, limit), res in got.items():
            same = np.nonzero((np.arange(n) + 3) % len(pool) == 3 % len(pool))[0]
            assert all(np.array_equal(res[key][i], got[1, 0][key][0], equal_nan=True) for i in same), (key, n, limit)
        assert np.array_equal(got[129, 0][key], got[129, small][key], equal_nan=True), key


@pytest.mark.gpu
@pytest.mark.skipif(not S.WIDE, reason="np.longdouble has fp64's exponent range here: no reference below 1e-308")
def test_the_scaled_mode_below_the_range_of_fp64(capi):
    pb = tree32(64, 70)[0]
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(70))
    fam = [0, 1, 2, capi.CAFE_FAMILY_ABSENT]
    want = GM.table(pb, fam, SCALED_RATES[0], pr.prior, 0.2, GM.LEVEL)
    assert want["lnl"][0] < -800 and want["cdf_gap"].min() > 1e-9 and want["top_gap"].min() > 1e-9
    with closing(capi.Context(pb)) as ctx:
        plain = ctx.gain_marginal_dense(pr, fam, *SCALED, 0.2, GM.LEVEL)
        assert plain["lnl"][0] == -np.inf and np.isnan(plain["mean"][0]).all() and (plain["mode"][0] == -1).all() and (plain["hi"][0] == -1).all()
        ctx.set_gain_scaling(True)
        got = ctx.gain_marginal_dense(pr, fam, *SCALED, 0.2, GM.LEVEL)
    assert all(np.array_equal(got[key], want[key]) for key in GM.INTS)
    print("scaled worst %.3g" % _close(got, want))
    assert np.abs(got["lnl"] - want["lnl"].astype(np.float64)).max() <= 1e-10 * np.abs(want["lnl"]).max()


@pytest.mark.gpu
def test_what_is_refused(capi):
    pb, pr = GM.problem(*GM.CASES[0])
    with closing(capi.Context(pb)) as ctx:
        for level in (0.0, 1.0, np.nan):
            with pytest.raises(capi.CafeError, match="code 1: cafe_gain_marginal_dense: level must lie in \\(0, 1\\)"):
                ctx.gain_marginal_dense(pr, [0], *RATES, GM.ABSENT, level)
    pb.counts[0, 0], pb.missing_counts = capi.CAFE_COUNT_MISSING, True
    with closing(capi.Context(pb)) as ctx:
        with pytest.raises(capi.CafeError, match="code 4: cafe_gain_marginal_dense: the table has missing cells"):
            ctx.gain_marginal_dense(pr, [0], *RATES, GM.ABSENT, GM.LEVEL)
