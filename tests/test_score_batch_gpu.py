"""cafe_score_batch: every point of a batch gets the BITS cafe_score gives that point on a second context of the same problem
(max_categories = the point's own K), whatever else stands in the batch.  Assertions are == on the doubles.

Shapes: matrix orders 41 (no extents, 16-deep K tiles) and 300 (extents, magnitude skip, K ranges) on the seven-species tree
and the tables of tests/missing_ref.py -- with every cell observed, and with its planned blanks --; tables of 5 distinct
families (fewer than one K4 workgroup of 16) and of 700 (three blocks of the final sum; a multiple of neither 16 nor 128)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import missing_ref as MR
from cafexp_amd import problem as P
from cafexp_amd.gamma_rates import discrete_gamma

pytestmark = pytest.mark.gpu

ORDERS = (41, 300)
RULES = ("max", "sum")
INF = float("inf")


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C_
    C_.load()
    return C_


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def problems():
    """(order, model, kind) -> problem; kind "full": every cell observed, "blank": missing_ref's blanks, 5 / 700: that many
    distinct families of order 41"""
    cache = {}

    def get(order, model="base", kind="full"):
        key = (order, model, kind)
        if key not in cache:
            if kind == "blank":
                counts = None
            elif kind == "full":
                counts = MR.table(order, blank=False)
            else:
                cap, rng = MR.SHAPES[order][2], np.random.default_rng(kind)        # a size per family, every species within 4 of it
                rows = np.unique(rng.integers(1, cap - 4, size=(3 * kind, 1)) + rng.integers(0, 5, size=(3 * kind, len(MR.SPECIES))), axis=0)
                counts = rows[np.random.default_rng(1).permutation(len(rows))[:kind]].astype(np.int32)
                assert len(counts) == kind and counts.sum(axis=1).min() > 0
            cache[key] = MR.problem(order, model, counts=counts)
        return cache[key]
    return get


def base_points(pb, G, n_lambdas=1, error_model=None):
    prior = P.prior_uniform(pb.max_root_family_size)
    lam = [(0.012 * (0.55 + 0.031 * g), 0.006 * (1.4 - 0.027 * g))[:n_lambdas] for g in range(G)]
    return [P.Params(lambdas=np.array(v), prior=prior, error_model=error_model) for v in lam]


def gamma_points(pb, G, K):
    pts, alphas = base_points(pb, G), [0.8 + 0.13 * g for g in range(G)]
    for pr, a in zip(pts, alphas):
        pr.cat_probs, pr.multipliers = discrete_gamma(K, a)
    return pts, alphas


def singles(capi, pb, points, alphas=None, mus=None, rule="max", ctx_mus=None, **kw):
    """score() of every point on ONE fresh context of the problem (its own K categories); mus: per point, set before its call"""
    K = 1 if points[0].multipliers is None else len(points[0].multipliers)
    ctx = capi.Context(pb, max_categories=K, **kw)
    try:
        ctx.set_root_rule(rule)
        if ctx_mus is not None:
            ctx.set_death_rates(ctx_mus)
        out = []
        for g, pr in enumerate(points):
            if mus is not None:
                ctx.set_death_rates(mus[g])
            out.append(ctx.score(pr, alpha=1.0 if alphas is None else alphas[g]))
        return np.array(out)
    finally:
        ctx.close()


def batch_context(capi, pb, points, rule="max", ctx_mus=None, slots=None, **kw):
    K = 1 if points[0].multipliers is None else len(points[0].multipliers)
    ctx = capi.Context(pb, max_categories=slots or len(points) * K, **kw)
    ctx.set_root_rule(rule)
    if ctx_mus is not None:
        ctx.set_death_rates(ctx_mus)
    return ctx


def check(capi, pb, points, alphas=None, mus=None, rules=RULES, ctx_mus=None, label="", **kw):
    for rule in rules:
        want = singles(capi, pb, points, alphas, mus, rule, ctx_mus, **kw)
        ctx = batch_context(capi, pb, points, rule, ctx_mus, **kw)
        try:
            got = ctx.score_batch(points, alphas=alphas, mus=mus)
        finally:
            ctx.close()
        print(label, rule, "batch", got[:4], "single", want[:4])
        assert np.isfinite(want).all(), (label, rule, want)
        assert bits(got) == bits(want), (label, rule, got, want)


# ------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize("G", (1, 2, 5, 32))
@pytest.mark.parametrize("order", ORDERS)
def test_base(capi, problems, order, G):
    pb = problems(order)
    check(capi, pb, base_points(pb, G), label="base order %d G %d" % (order, G))


@pytest.mark.parametrize("K,G", ((3, 2), (3, 10), (8, 4)))
@pytest.mark.parametrize("order", ORDERS)
def test_gamma(capi, problems, order, K, G):
    pb = problems(order)
    pts, alphas = gamma_points(pb, G, K)
    check(capi, pb, pts, alphas, label="gamma order %d K %d G %d" % (order, K, G))


@pytest.mark.parametrize("order", ORDERS)
def test_two_lambdas(capi, problems, order):
    pb = problems(order, "two_lambdas")
    check(capi, pb, base_points(pb, 3, n_lambdas=2), label="two lambdas order %d" % order)


@pytest.mark.parametrize("order", ORDERS)
def test_death_rates_per_point_and_of_the_context(capi, problems, order):
    pb = problems(order, "death_rates")
    pts = base_points(pb, 4, n_lambdas=2)
    mus = np.array([[0.007, 0.009], [0.0065, 0.0031], [0.012, 0.002], [0.0071, 0.0088]])
    check(capi, pb, pts, mus=mus, ctx_mus=MR.MUS, label="mus per point order %d" % order)
    check(capi, pb, pts, ctx_mus=MR.MUS, label="the context's mus order %d" % order)
    ctx = batch_context(capi, pb, pts, ctx_mus=MR.MUS)
    try:                                     # the batch left the context's own death rates alone
        ctx.score_batch(pts, mus=mus)
        after = ctx.score(pts[0])
    finally:
        ctx.close()
    assert bits(after) == bits(singles(capi, pb, pts[:1], ctx_mus=MR.MUS))


@pytest.mark.parametrize("order", ORDERS)
def test_error_model_of_three_taps(capi, problems, order):
    pb = problems(order, "error3")
    check(capi, pb, base_points(pb, 3, error_model=MR.error_model(pb.max_family_size, 3)), label="error3 order %d" % order)


@pytest.mark.parametrize("order", ORDERS)
def test_missing_cells(capi, problems, order):
    pb = problems(order, kind="blank")
    assert pb.missing_counts
    check(capi, pb, base_points(pb, 3), label="missing base order %d" % order)
    pts, alphas = gamma_points(pb, 2, 3)
    check(capi, pb, pts, alphas, label="missing gamma order %d" % order)


@pytest.mark.parametrize("n", (5, 700))
def test_family_counts_around_the_reductions_blocks(capi, problems, n):
    pb = problems(41, kind=n)
    assert pb.n_families == n
    check(capi, pb, base_points(pb, 5), label="%d families base" % n)
    pts, alphas = gamma_points(pb, 2, 3)
    check(capi, pb, pts, alphas, label="%d families gamma" % n)


# ------------------------------------------------------------------------------------------------ the contexts
@pytest.mark.parametrize("order", ORDERS)
def test_one_op_per_launch(capi, problems, monkeypatch, order):
    pb = problems(order)
    monkeypatch.setenv("CAFE_NO_GROUPS", "1")
    pts, alphas = gamma_points(pb, 3, 3)
    check(capi, pb, pts, alphas, rules=("max",), label="no groups order %d" % order)


def test_several_column_chunks(capi, problems):
    pb = problems(41, kind=700)
    pts, alphas = gamma_points(pb, 2, 3)
    want = singles(capi, pb, pts, alphas)
    chunks = 0
    for limit in (8 << 20, 4 << 20, 2 << 20, 1 << 20, 512 << 10):
        try:
            ctx = batch_context(capi, pb, pts, workspace_limit=limit)
        except capi.CafeError:
            continue
        try:
            got = ctx.score_batch(pts, alphas=alphas)
            chunks = max(chunks, ctx.stats()["n_chunks"])
        finally:
            ctx.close()
        assert bits(got) == bits(want), (limit, got, want)
    assert chunks >= 3, chunks


@pytest.mark.parametrize("order", ORDERS)
def test_graphs_on(capi, problems, order):
    pb = problems(order)
    pts, alphas = gamma_points(pb, 4, 3)
    want = singles(capi, pb, pts, alphas)
    ctx = batch_context(capi, pb, pts)
    try:
        ctx.set_graphs(True)
        first = ctx.score_batch(pts, alphas=alphas)                   # captured
        again = ctx.score_batch(pts, alphas=alphas)                   # replayed
        fewer = ctx.score_batch(pts[1:3], alphas=alphas[1:3])         # another G: a graph of its own
        ctx.set_graphs(False)
        plain = ctx.score_batch(pts, alphas=alphas)
    finally:
        ctx.close()
    assert bits(first) == bits(want) and bits(again) == bits(want) and bits(plain) == bits(want)
    assert bits(fewer) == bits(want[1:3])


# ------------------------------------------------------------------------------------------------ inside a batch
@pytest.mark.parametrize("order", ORDERS)
def test_rejected_equal_and_permuted_points(capi, problems, order):
    pb = problems(order)
    pts, alphas = gamma_points(pb, 6, 3)
    want = singles(capi, pb, pts, alphas)
    bad_lambda = dataclasses.replace(pts[0], lambdas=np.array([0.0]))
    neg_lambda = dataclasses.replace(pts[0], lambdas=np.array([-0.01]))
    zero_cat = dataclasses.replace(pts[1], multipliers=np.array([1e-12, 1.0, 2.0]))   # lambda x multiplier quantizes to 0: that category's root vectors are 0
    assert singles(capi, pb, [zero_cat], [alphas[1]])[0] == INF
    ctx = batch_context(capi, pb, pts, slots=30)
    try:
        # (point, alpha) lists; the expected value of every entry
        mixed = [(pts[0], alphas[0]), (bad_lambda, 1.0), (pts[1], alphas[1]), (pts[2], -0.5), (zero_cat, alphas[1]), (pts[3], alphas[3]),
                 (pts[1], alphas[1]), (neg_lambda, 1.0)]
        expect = np.array([want[0], INF, want[1], INF, INF, want[3], want[1], INF])
        got = ctx.score_batch([p for p, _ in mixed], alphas=[a for _, a in mixed])
        assert bits(got) == bits(expect), (got, expect)
        perm = [5, 2, 7, 0, 4, 6, 1, 3]
        got = ctx.score_batch([mixed[i][0] for i in perm], alphas=[mixed[i][1] for i in perm])
        assert bits(got) == bits(expect[perm]), (got, expect[perm])
        # only rejected points: +inf each, nothing launched
        got = ctx.score_batch([bad_lambda, pts[2], neg_lambda], alphas=[1.0, -1.0, 1.0])
        assert bits(got) == bits([INF, INF, INF])
        st = ctx.stats()
        assert st["gemm_launches"] == 0 and st["n_matrices"] == 0, st
        with pytest.raises(capi.CafeError, match="code 4"):
            ctx.family_results(3)
        # the base model's rejection: lambda <= 0 alone
        b = base_points(pb, 3)
        got = ctx.score_batch([b[0], dataclasses.replace(b[1], lambdas=np.array([0.0])), b[2]])
        wb = singles(capi, pb, b)
        assert bits(got) == bits([wb[0], INF, wb[2]])
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ORDERS)
def test_after_a_batch(capi, problems, order):
    pb = problems(order)
    pts, alphas = gamma_points(pb, 3, 3)
    fresh = capi.Context(pb, max_categories=3)
    try:
        want, want_fam = fresh.score(pts[1], alpha=alphas[1], per_family=True)
    finally:
        fresh.close()
    ctx = batch_context(capi, pb, pts)
    try:
        ctx.score_batch(pts, alphas=alphas)
        with pytest.raises(capi.CafeError, match="code 4"):
            ctx.family_results(3)
        with pytest.raises(capi.CafeError, match="code 4"):
            ctx.matrix(1)
        got, fam = ctx.score(pts[1], alpha=alphas[1], per_family=True)
        assert bits(got) == bits(want)
        for key in want_fam:
            assert bits(fam[key]) == bits(want_fam[key]), key
    finally:
        ctx.close()


def test_argument_and_state_errors(capi, problems):
    pb = problems(41)
    pts, alphas = gamma_points(pb, 11, 3)
    ctx = capi.Context(pb, max_categories=32)
    try:
        with pytest.raises(capi.CafeError, match="code 1.*max_categories"):
            ctx.score_batch(pts, alphas=alphas)                     # 11 x 3 = 33
        with pytest.raises(capi.CafeError, match="code 1.*max_categories"):
            ctx.score_batch(base_points(pb, 33))
        with pytest.raises(capi.CafeError, match="code 4.*death rates"):
            ctx.score_batch(base_points(pb, 2), mus=[[0.01], [0.02]])
        lib = capi.load()
        out = np.zeros(2)
        f64p = C.POINTER(C.c_double)
        assert lib.cafe_score_batch(ctx._h, None, out.ctypes.data_as(f64p)) == 1
        bp = capi.CafeBatchParams()
        assert lib.cafe_score_batch(ctx._h, C.byref(bp), None) == 1
        assert lib.cafe_score_batch(None, C.byref(bp), out.ctypes.data_as(f64p)) == 1
        bp.n_points, bp.model, bp.n_categories = 2, capi.CAFE_MODEL_BASE, 1
        assert lib.cafe_score_batch(ctx._h, C.byref(bp), out.ctypes.data_as(f64p)) == 1       # no lambdas, no prior
        # the context is as good as new
        one = base_points(pb, 1)
        assert bits(ctx.score_batch(one)) == bits(singles(capi, pb, one))
    finally:
        ctx.close()
