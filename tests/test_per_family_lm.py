"""cafe_score_per_family_lm (family_lambda_kernel.h on SlotParamLM, family_lambda_lm.hip): the per-family kernel under separate
birth and death rates, every family of a call under its own (lambdas, mus).

References: the scorer path of the same context under cafe_set_death_rates (tests/test_bd_lm_gpu.py pins it to a numpy prune),
one call per distinct pair, and that numpy prune itself on the matrices of tests/bd_lm_ref.py.  Tolerance: the per-family one,
test_lambda_per_family._close at REL = 1e-10, infinities matched exactly.  With mus == lambdas the values are compared with
cafe_score_per_family's by ==: the kernel is one body for both slot types, bd_row_step with a == b runs the equal-rate form's
operands, and slot_param_lm takes K1's formula at equal quantized rates."""
import dataclasses

import numpy as np
import pytest

import bd_lm_ref as R
import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import _explicit_problem
from test_lambda_per_family import _close
from test_per_family_shapes import ORDERS, TREE3, WIDTHS, families, sizes, width

# lambda / mu = 0.25, 0.8, 1.25, 4: one pair per family of the three-taxon table
PAIRS = [(0.0011, 0.0044), (0.002, 0.0025), (0.0051, 0.00408), (0.0034, 0.00085)]
RATIOS = (0.25, 0.8, 1.25, 4.0)


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _params(pb, error=False):
    return R.params(pb, "error" if error else "base")


def _scorer_per_pair(ctx, pr, fam, lam, mu):
    """family fam[i] under (lam[i], mu[i]) by the scorer path: set_death_rates + score(per_family=True), once per distinct pair"""
    want = np.empty(len(fam))
    both = np.concatenate([lam, mu], axis=1)
    L = lam.shape[1]
    try:
        for vec in np.unique(both, axis=0):
            sel = np.all(both == vec, axis=1)
            ctx.set_death_rates(vec[L:])
            if not (np.all(vec[L:] >= 0) and (vec[0] > 0 if L == 1 else not np.any(vec[:L] < 0))):
                assert ctx.score(dataclasses.replace(pr, lambdas=vec[:L].copy())) == np.inf      # rejected on the host: no family results
                want[sel] = -np.inf
                continue
            _, res = ctx.score(dataclasses.replace(pr, lambdas=vec[:L].copy()), per_family=True)
            want[sel] = res["family_lnl"][np.asarray(fam)[sel]]
    finally:
        ctx.set_death_rates(None)
    return want


# ------------------------------------------------------------------ the numpy prune of the six-taxon problem (bd_lm_ref.py)
def context_pairs(pb):
    """One (lambdas, mus) per family of bd_lm_ref.problem: drawn around LAMBDAS / MUS, family 0 pure death, family 1 pure birth"""
    rng = np.random.default_rng(pb.matrix_size)
    lam = R.LAMBDAS * rng.uniform(0.6, 1.5, size=(pb.n_families, 2))
    mu = R.MUS * rng.uniform(0.6, 1.5, size=(pb.n_families, 2))
    lam[0] = 0.0
    mu[1] = 0.0
    return lam, mu


def numpy_prune(pb, pr, lam, mu):
    """lnL of family f under (lam[f], mu[f]): the up pass of tests/marginal_ref.py on bd_lm_ref.matrix, the base model's reduction"""
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)
    out = np.empty(pb.n_families)
    for f in range(pb.n_families):
        one = dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[f:f + 1]), family_ids=pb.family_ids[f:f + 1])
        inside = MR.updown(one, pr, R.reference_matrices(pb, lam[f], mu[f], [1.0]), 0.95)["root_inside"][0][0]
        with np.errstate(divide="ignore"):
            out[f] = np.max(np.log(inside) + np.log(prior))
    return out


_prunes = {}


def prune_case(order, error, which="right"):
    key = (order, error, which)
    if key not in _prunes:
        pb = R.problem(order, n_dev=3 if error else 0)
        lam, mu = context_pairs(pb)
        args = {"right": (lam, mu), "exchanged": (mu, lam), "mu_ignored": (lam, lam)}[which]
        _prunes[key] = numpy_prune(pb, _params(pb, error), *args)
    return _prunes[key]


# ------------------------------------------------------------------ CPU
def test_the_orders_reach_every_instantiation():
    assert {width(n) for n in ORDERS} == set(WIDTHS)
    for lo, hi in zip(WIDTHS, WIDTHS[1:]):                   # both sides of every switch of the ladder
        assert 64 * lo in ORDERS and width(64 * lo) == lo
        assert 64 * lo + 1 in ORDERS and width(64 * lo + 1) == hi
    assert {3, 16, 17, 33, 2047, 2048} <= set(ORDERS) and width(2048) == 32
    for (lam, mu), rho in zip(PAIRS, RATIOS):
        assert lam / mu == pytest.approx(rho, rel=1e-12)


@pytest.mark.parametrize("order", [41, 300])
def test_the_inputs_tell_an_exchanged_and_an_ignored_mu_apart(order):
    right = prune_case(order, False)
    finite = np.isfinite(right)
    assert finite.sum() >= 6
    for which in ("exchanged", "mu_ignored"):
        wrong = prune_case(order, False, which)
        both = finite & np.isfinite(wrong)
        rel = np.abs(wrong[both] - right[both]) / np.abs(right[both])
        print("order %d %s: relative differences %s" % (order, which, rel))
        # every family whose value stays finite moves by far more than the GPU test's 1e-10 (pure birth / death may turn -inf)
        assert np.all(rel > 1e-6) and both.sum() >= 5, (which, rel)


@pytest.mark.parametrize("order", [41, 300])
def test_the_error_model_inputs_tell_them_apart_too(order):
    right = prune_case(order, True)
    for which in ("exchanged", "mu_ignored"):
        wrong = prune_case(order, True, which)
        both = np.isfinite(right) & np.isfinite(wrong)
        rel = np.abs(wrong[both] - right[both]) / np.abs(right[both])
        print("order %d, error model, %s: relative differences %s" % (order, which, rel))
        assert np.all(rel > 1e-6) and both.sum() >= 5, (which, rel)


@pytest.mark.parametrize("n", [3, 33, 129])
def test_the_every_width_pairs_tell_them_apart(n):
    """The four (lambda, mu) of the every-width test on its own tree and families, at three of its orders: the numpy prune with the
    rates exchanged, and with mu = lambda, misses the right value of every family by more than 1e-6 relative."""
    M, Rr = sizes(n)
    pb = _explicit_problem(TREE3, families(n), M, Rr)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    lam, mu = np.array(PAIRS)[:, :1], np.array(PAIRS)[:, 1:]
    right = numpy_prune(pb, pr, lam, mu)
    assert np.isfinite(right).all()
    for which, args in (("exchanged", (mu, lam)), ("mu_ignored", (lam, lam))):
        wrong = numpy_prune(pb, pr, *args)
        rel = np.abs(wrong - right) / np.abs(right)
        print("n %d %s: relative differences %s" % (n, which, rel))
        assert np.all(rel > 1e-6), (which, rel)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", ORDERS)
def test_every_width_against_the_scorer_under_death_rates(capi, n):
    M, Rr = sizes(n)
    pb = _explicit_problem(TREE3, families(n), M, Rr)
    assert pb.matrix_size == n and pb.n_families == 4
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    lam, mu = np.array(PAIRS)[:, :1], np.array(PAIRS)[:, 1:]
    fam = np.arange(4)
    ctx = capi.Context(pb)
    try:
        got = ctx.score_per_family_lm(pr, fam, lam, mu)
        want = _scorer_per_pair(ctx, pr, fam, lam, mu)
    finally:
        ctx.close()
    print("n %d E %d: lnL %s" % (n, width(n), got))
    _close(got, want)
    assert np.isfinite(got).all()


@pytest.mark.gpu
@pytest.mark.parametrize("error", [False, True])
@pytest.mark.parametrize("order", [41, 300])
def test_against_the_numpy_prune(capi, order, error):
    pb = R.problem(order, n_dev=3 if error else 0)
    pr = _params(pb, error)
    lam, mu = context_pairs(pb)
    want = prune_case(order, error)
    ctx = capi.Context(pb)
    try:
        got = ctx.score_per_family_lm(pr, np.arange(pb.n_families), lam, mu)
        scorer = _scorer_per_pair(ctx, pr, np.arange(pb.n_families), lam, mu)
    finally:
        ctx.close()
    print("order %d error %s: lnL %s" % (order, error, got))
    assert np.isfinite(want).sum() >= 6
    _close(got, want)
    _close(got, scorer)


def _equal_rates_case(capi, n, error):
    M, Rr = sizes(n)
    rows = families(n)
    tree = P.parse_newick(TREE3)
    species = sorted(rows[0])
    table = np.array([[r[s] for s in species] for r in rows], dtype=np.int32)
    pb = P.build_problem(tree, species, ["f%d" % i for i in range(4)], table, root_filter=False, max_family_size=M,
                         max_root_family_size=Rr, n_deviations=3 if error else 0)
    em = None
    if error:
        em = np.tile(np.array([0.05, 0.9, 0.05]), (M + 1, 1))
        em[0] = [0.0, 0.95, 0.05]
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr), error_model=em)
    lam = np.array([p[0] for p in PAIRS])
    ctx = capi.Context(pb)
    try:
        plain = ctx.score_per_family(pr, np.arange(4), lam)
        twin = ctx.score_per_family_lm(pr, np.arange(4), lam, lam)
        other = ctx.score_per_family_lm(pr, np.arange(4), lam, 0.7 * lam)
    finally:
        ctx.close()
    assert np.isfinite(plain).all()
    assert np.array_equal(twin, plain)
    assert not np.any(other == plain)                        # the second rate is read


@pytest.mark.gpu
@pytest.mark.parametrize("error", [False, True])
@pytest.mark.parametrize("n", [33, 641, 2048])
def test_equal_rates_are_the_lambda_only_entry_bit_for_bit(capi, n, error):
    _equal_rates_case(capi, n, error)


# one order per instantiation of the kernel (the smallest that selects the width, and the maximum); the error model at the
# first, a middle and the last
EVERY_WIDTH = [128, 129, 257, 385, 513, 641, 769, 897, 1025, 1281, 1537, 1793, 2048]


@pytest.mark.gpu
@pytest.mark.parametrize("n,error", [(n, False) for n in EVERY_WIDTH] + [(n, True) for n in (128, 641, 2048)])
def test_equal_rates_are_the_lambda_only_entry_at_every_width(capi, n, error):
    assert sorted({width(m) for m in EVERY_WIDTH}) == WIDTHS
    _equal_rates_case(capi, n, error)


@pytest.mark.gpu
def test_values_the_host_decides(capi):
    pb = R.problem(41)
    pr = _params(pb)
    F = pb.n_families
    longest = float(np.max(pb.branch_length[np.asarray(pb.parent) >= 0]))
    lam, mu = np.tile(R.LAMBDAS, (F, 1)), np.tile(R.MUS, (F, 1))
    sat = np.array(R.SATURATED[:2]) * R.SATURATED[2] / longest      # the same lambda t, mu t on the tree's longest branch
    assert R.rates(sat[0], sat[1], longest)[2]
    mu[1, 1] = -1e-9                                         # a negative mu: -inf
    lam[2, 0] = np.nan                                       # several lambdas: a NaN is not negative, it passes and gives NaN
    lam[3], mu[3] = sat[0], sat[1]                           # saturated on the long branches: what the scorer gives
    mu[4, 0] = np.nan                                        # a NaN mu fails mu >= 0, as it does in the scorer
    ctx = capi.Context(pb)
    try:
        fam = np.arange(F)
        valid = ctx.score_per_family_lm(pr, fam, np.tile(R.LAMBDAS, (F, 1)), np.tile(R.MUS, (F, 1)))
        got = ctx.score_per_family_lm(pr, fam, lam, mu)
        for i in (1, 2, 3, 4):                               # alone
            assert np.array_equal(ctx.score_per_family_lm(pr, [i], lam[i:i + 1], mu[i:i + 1]), got[i:i + 1], equal_nan=True), i
        keep = np.array([0, 5, 6, 7])
        want = _scorer_per_pair(ctx, pr, fam[[1, 3]], lam[[1, 3]], mu[[1, 3]])
        ctx.set_death_rates(mu[4])                           # (a NaN has no place in the helper's table of distinct pairs)
        assert ctx.score(dataclasses.replace(pr, lambdas=lam[4].copy())) == np.inf
        # the context's own death rates are not read
        ctx.set_death_rates(3 * R.MUS)
        assert np.array_equal(ctx.score_per_family_lm(pr, fam, lam, mu), got, equal_nan=True)
        with pytest.raises(capi.CafeError, match="code 4"):  # the lambda = mu entry still refuses
            ctx.score_per_family(pr, [0], R.LAMBDAS[None])
        ctx.set_death_rates(None)
        gamma = R.params(pb, "gamma")
        with pytest.raises(capi.CafeError, match="code 1"):  # CAFE_ERR_ARGUMENT: base model only
            ctx.score_per_family_lm(gamma, [0], R.LAMBDAS[None], R.MUS[None])
    finally:
        ctx.close()
    print("mixed call: %s\nscorer for entries 1, 3: %s" % (got, want))
    assert np.isfinite(valid).all() and np.array_equal(got[keep], valid[keep])
    assert got[1] == -np.inf and np.isnan(got[2]) and got[4] == -np.inf
    assert want[0] == -np.inf
    _close(got[[3]], want[[1]])

    # one lambda: lambda = 0 is invalid
    M, Rr = sizes(33)
    one = _explicit_problem(TREE3, families(33), M, Rr)
    ctx = capi.Context(one)
    try:
        got = ctx.score_per_family_lm(P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr)), [0, 1], [0.0, 0.002], [0.001, 0.001])
    finally:
        ctx.close()
    assert got[0] == -np.inf and np.isfinite(got[1])


@pytest.mark.gpu
def test_batch_cut_at_a_wide_order(capi):
    n = 1281
    assert n >= 1025 and width(n) >= 20
    M, Rr = sizes(n)
    pb = _explicit_problem(TREE3, families(n) + [{"A": 7, "B": 0, "C": 3}, {"A": 120, "B": 111, "C": 130}, {"A": 1, "B": 1, "C": 1}], M, Rr)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    limit, reps = 16 << 20, 1200
    # a listed family takes at least n_nodes * ld doubles of factors, so a batch holds at most limit / that many
    assert reps * pb.n_nodes * n * 8 >= 3 * limit
    fam = np.arange(reps) % pb.n_families
    lam = np.array([p[0] for p in PAIRS])[np.arange(reps) % 4]
    mu = np.array([p[1] for p in PAIRS])[np.arange(reps) % 4]
    results = []
    for ws in (limit, 0):
        ctx = capi.Context(pb, workspace_limit=ws)
        try:
            results.append(ctx.score_per_family_lm(pr, fam, lam, mu))
        finally:
            ctx.close()
    assert np.isfinite(results[0]).all()
    assert np.array_equal(results[0], results[1])
    assert np.array_equal(results[0][:28], results[0][28:56])             # the list repeats every 28 entries: so do the values
