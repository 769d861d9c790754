"""cafe_branch_scores (csrc/branch_scores.hip on gradient.hip's walk) at the shapes of tests/test_gradient_shapes.py: its
tree, (M, R) pairs, count rows and three configurations, imported from it.

Reference and bound: branch_scores_ref.reverse, every entry of rate / birth / death held by gradient_ref.close to
|got - ref| <= 1e-12 + 1e-10 c |ref| with c the reference's own cancellation factor of that entry, at most C_BOUND.  The
largest factor the reference reports on these inputs is asserted on the CPU to lie in (C_BOUND / 10, C_BOUND]
(test_the_reference_reports_the_cancellation_the_bound_assumes prints it per configuration).

Three column batches, a saturated branch, mus == lambdas against the unset call, failed families."""
import functools

import numpy as np
import pytest

import branch_scores_ref as BR
import gradient_ref as GR
import test_gradient_shapes as TS
from test_gradient_shapes import COLUMNS, CONFIGS, LAMBDAS, PAIRS, kBN

C_BOUND = 1e5
EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def pair_case(M, R, config, rule):
    pb, pr, mus, _ = TS._pair_case(M, R, config, rule)
    return pb, pr, mus, BR.reverse(pb, pr, mus, rule)


@functools.lru_cache(maxsize=None)
def column_case(n, rule="max"):
    pb, pr, mus, _ = TS._column_case(n, rule)
    return pb, pr, mus, BR.reverse(pb, pr, mus, rule)


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_reference_reports_the_cancellation_the_bound_assumes(config):
    worst = max(BR.worst_cancellation(pair_case(M, R, config, rule)[3]) for M, R in PAIRS for rule in ("max", "sum"))
    print("%s: largest cancellation factor of a branch score over the pairs %.1f" % (config, worst))
    assert worst <= C_BOUND
    if config == "gamma_err_rho_0.25":
        cols = max(BR.worst_cancellation(column_case(n)[3]) for n in COLUMNS)
        print("largest cancellation factor over the column counts %.1f" % cols)
        assert cols <= C_BOUND


def test_the_bound_is_the_power_of_ten_above_the_largest_factor():
    worst = max(BR.worst_cancellation(pair_case(M, R, config, rule)[3]) for config in CONFIGS for M, R in PAIRS for rule in ("max", "sum"))
    worst = max(worst, max(BR.worst_cancellation(column_case(n)[3]) for n in COLUMNS))
    assert C_BOUND / 10 < worst <= C_BOUND, worst


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def run(capi, pb, pr, mus, rule, ref, label, **ctx_args):
    """one cafe_branch_scores call held to the reference; -> (its result, cafe_score_gradient's from the same context)"""
    ctx = capi.Context(pb, max_categories=TS._K(pr), **ctx_args)
    try:
        ctx.set_death_rates(mus)
        got = ctx.branch_scores(pr, rule, alpha=0.7)
        grad = ctx.score_gradient(pr, rule, alpha=0.7)
    finally:
        ctx.close()
    GR.close(BR.as_gradient(got), BR.as_gradient(ref), C_BOUND, label)
    for key in ("family_lnl", "failed") + GR.KEYS:           # one body: the global scores are cafe_score_gradient's bits
        assert (key in got) == (key in grad), (label, key)
        if key in grad:
            assert np.array_equal(got[key], grad[key], equal_nan=True), (label, key)
    check_gram(got, pb, 1 if mus is None else 2, label)
    return got, grad


def check_gram(got, pb, n_par, label):
    """gram and total against numpy (extended precision) from the returned rows: a sum of n products in any order differs from
    the exact one by at most n eps times the sum of the absolute products, for either side: 2 n eps (|S|^T W |S|)_ij, n the
    distinct families"""
    z = BR.score_vectors(got, pb, n_par)
    assert z.shape[1] == got["gram"].shape[0] == got["total"].shape[0], label
    total, gram, absgram, used = BR.gram_of(z, got["failed"])
    n = len(np.unique(pb.counts, axis=0))
    assert got["n_used"] == used, label
    assert np.array_equal(got["gram"], got["gram"].T), label
    room = 2 * n * EPS * absgram
    err = np.abs(got["gram"] - gram)
    print("%s: worst |gram - numpy| / bound %.3g" % (label, np.max(err[room > 0] / room[room > 0]) if (room > 0).any() else 0.0))
    assert np.all(err <= room), label
    zz = np.abs(z[got["failed"] == 0]).astype(np.longdouble)
    assert np.all(np.abs(got["total"] - total) <= 2 * n * EPS * zz.sum(axis=0)), label


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("M,R", PAIRS)
def test_every_pair_model_and_rule(capi, M, R, config):
    for rule in ("max", "sum"):
        pb, pr, mus, ref = pair_case(M, R, config, rule)
        got, _ = run(capi, pb, pr, mus, rule, ref, "M %d R %d %s %s" % (M, R, config, rule))
        assert not got["failed"].any()
        root = int(np.flatnonzero(pb.parent < 0)[0])
        for key in BR.NAMES:
            if key in got:
                assert np.all(np.isnan(got[key][:, root])) and not np.isnan(np.delete(got[key], root, axis=1)).any(), key
                assert np.array_equal(got[key][4], got[key][2], equal_nan=True) and np.array_equal(got[key][5], got[key][0], equal_nan=True), key
        assert ("birth" in got) == (mus is not None)
        if mus is not None:
            assert np.array_equal(got["rate"], got["birth"] + got["death"], equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", COLUMNS)
def test_column_counts_around_the_tile(capi, n):
    pb, pr, mus, ref = column_case(n)
    run(capi, pb, pr, mus, "max", ref, "%d distinct families" % n)


@pytest.mark.gpu
def test_three_column_batches_change_no_bit(capi):
    pb, pr, mus, ref = column_case(300)
    per_col = TS._per_col(pb, 3, 2)                          # the walk's workspace per column is cafe_score_gradient's: the panel is not in it
    limit = kBN * per_col + per_col // 2
    assert limit // per_col // kBN * kBN == kBN and -(-300 // kBN) == 3
    want, _ = run(capi, pb, pr, mus, "max", ref, "one batch")
    got, _ = run(capi, pb, pr, mus, "max", ref, "three batches", workspace_limit=limit)
    assert {"rate", "birth", "death", "total", "gram", "n_used"} <= set(want)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["base", "gamma"])
def test_equal_death_rates_give_the_unset_rate(capi, config):
    cfg = dict(model=config, err=True, mus=None)
    pb = TS._problem(40, 30, err=True)
    pr = TS._params(pb, cfg)
    ctx = capi.Context(pb, max_categories=TS._K(pr))
    try:
        for rule in ("max", "sum"):
            one = ctx.branch_scores(pr, rule, alpha=0.7)
            ctx.set_death_rates(LAMBDAS)
            both = ctx.branch_scores(pr, rule, alpha=0.7)
            ctx.set_death_rates(None)
            two, unset = BR.reverse(pb, pr, LAMBDAS, rule), BR.reverse(pb, pr, None, rule)
            ok = ~np.isnan(unset["rate"])
            # entry by entry: 1e-10 of the sums of |terms| behind the two numbers
            room = (two["cancel_rate"] * np.abs(two["rate"]) + unset["cancel_rate"] * np.abs(unset["rate"]))[ok]
            diff = np.abs(both["rate"] - one["rate"])[ok]
            print("%s %s: worst |rate(mus == lambdas) - rate(unset)| / bound %.3g" % (config, rule, np.max(diff / (1e-12 + 1e-10 * room))))
            assert np.all(diff <= 1e-12 + 1e-10 * room), rule
            assert np.array_equal(both["family_lnl"], one["family_lnl"])
            assert "birth" in both and "birth" not in one
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_saturated_branch_and_failed_families(capi):
    """TS._saturated_case: lambda_2 t = 1.2 on A's branch (zero-marked), and every family with A or B above 0 fails"""
    pb, pr, possible = TS._saturated_case()
    sat = int(np.flatnonzero(pb.lambda_index == 1)[0])
    root = int(np.flatnonzero(pb.parent < 0)[0])
    nonroot = [v for v in range(pb.n_nodes) if v != root]
    for rule in ("max", "sum"):
        ref = BR.reverse(pb, pr, None, rule)
        got, _ = run(capi, pb, pr, None, rule, ref, "saturated %s" % rule)
        assert np.array_equal(got["failed"] == 0, possible)
        assert np.all(got["rate"][possible, sat] == 0.0)
        assert np.any(got["rate"][possible][:, [v for v in nonroot if v != sat]] != 0.0)
        assert np.all(np.isnan(got["rate"][~possible]))      # a failed family: NaN in its rows ...
        assert got["n_used"] == possible.sum()               # ... and absent from total / gram
        i = nonroot.index(sat)
        assert np.all(got["gram"][i] == 0.0) and np.all(got["gram"][:, i] == 0.0) and got["total"][i] == 0.0
        assert np.isfinite(got["gram"]).all() and np.isfinite(got["total"]).all()
