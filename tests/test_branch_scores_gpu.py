"""cafe_branch_scores and cafe_weighted_gram on the GPU, beside the shapes of tests/test_branch_scores_shapes.py:

  * an independent cross-check through existing code: a second context over the same table whose lambda tree gives every
    branch its own index; its cafe_score_gradient must satisfy lambda d_lambda[f][index(v)] (+ mu d_mu) = rate[f][v] under
    the parity bound (every entry to the reference's own cancellation factor, at most C_BOUND);
  * the GEMM launches and flops of cafe_branch_scores are cafe_score_gradient's;
  * NULL outputs, the state error of birth / death without death rates, cafe_branch_scores_dim;
  * cafe_weighted_gram alone at P in {1, 15, 16, 17, 33} and n in {1, 3, 4, 5, slab - 1, slab, slab + 1, 2 slab + 3}, weights
    with zeros and non-integers, against numpy (in extended precision) under |got - ref|_ij <= 2 n eps (|S| W |S|^T)_ij -- the bound of a sum of n
    products in any order, for either side --, exactly symmetric, identical bits from two calls, NaN under a zero weight."""
import re

import numpy as np
import pytest

import branch_scores_ref as BR
import gradient_ref as GR
import test_gradient_shapes as TS
from cafexp_amd import problem as P
from test_branch_scores_shapes import C_BOUND, EPS, capi, pair_case  # noqa: F401  (capi: the fixture)

SLAB = 2048                                                  # kGramSlab of csrc/branch_scores.hip


def own_index_lambda_tree():
    """TS.TREE with every branch length replaced by a label of its own, 1, 2, ... in the order of the text"""
    count = [0]

    def label(_):
        count[0] += 1
        return ":%d" % count[0]
    text = re.sub(r":[0-9.]+", label, TS.TREE)
    return text, count[0]


def test_the_own_index_tree_has_one_index_per_branch():
    text, n = own_index_lambda_tree()
    pb = TS._problem(16, 14)
    assert n == pb.n_nodes - 1
    pb2 = own_index_problem(pb, 16, 14, False)
    assert pb2.n_lambdas == n and sorted(pb2.lambda_index[pb2.parent >= 0]) == list(range(n))
    assert np.array_equal(pb2.parent, pb.parent) and np.array_equal(pb2.counts, pb.counts)


def own_index_problem(pb, M, R, err):
    text, _ = own_index_lambda_tree()
    return P.build_problem(P.parse_newick(TS.TREE), TS.SPECIES, list(pb.family_ids), pb.counts, lambda_tree=P.parse_newick(text, lambda_tree=True),
                           root_filter=False, max_family_size=M, max_root_family_size=R, n_deviations=3 if err else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("rates", ["equal", "classes"])
@pytest.mark.parametrize("config", sorted(TS.CONFIGS))
def test_one_lambda_per_branch_through_the_gradient_call(capi, config, rates):
    M, R = 16, 40
    cfg = TS.CONFIGS[config]
    pb = TS._problem(M, R, err=cfg["err"])
    pr = TS._params(pb, cfg)
    mus = cfg["mus"]
    if rates == "equal":                                     # all lambda equal (and all mu)
        pr.lambdas = np.full(2, TS.LAMBDAS[0])
        mus = None if mus is None else np.full(2, mus[0])
    pb2 = own_index_problem(pb, M, R, cfg["err"])
    nonroot = np.flatnonzero(pb.parent >= 0)
    idx = pb2.lambda_index[nonroot]
    pr2 = TS._params(pb2, cfg)
    pr2.lambdas = np.empty(pb2.n_lambdas)
    pr2.lambdas[idx] = pr.lambdas[pb.lambda_index[nonroot]]
    mus2 = None
    if mus is not None:
        mus2 = np.empty(pb2.n_lambdas)
        mus2[idx] = mus[pb.lambda_index[nonroot]]
    for rule in ("max", "sum"):
        ref = BR.reverse(pb, pr, mus, rule)
        assert BR.worst_cancellation(ref) <= C_BOUND
        a, b = capi.Context(pb, max_categories=TS._K(pr)), capi.Context(pb2, max_categories=TS._K(pr))
        try:
            a.set_death_rates(mus)
            b.set_death_rates(mus2)
            got = a.branch_scores(pr, rule, alpha=0.7, gram=False)
            grad = b.score_gradient(pr2, rule, alpha=0.7)
        finally:
            a.close()
            b.close()
        assert np.array_equal(got["family_lnl"], grad["family_lnl"])
        through = np.full(got["rate"].shape, np.nan)
        through[:, nonroot] = pr2.lambdas[idx] * grad["d_lambda"][:, idx]
        if mus is not None:
            through[:, nonroot] += mus2[idx] * grad["d_mu"][:, idx]
        label = "%s %s %s" % (config, rates, rule)
        GR.close({"failed": grad["failed"], "d_lambda": through}, {"failed": ref["failed"], "d_lambda": ref["rate"], "cancel_d_lambda": ref["cancel_rate"]},
                 C_BOUND, "own index, through cafe_score_gradient: " + label)
        GR.close({"failed": got["failed"], "d_lambda": got["rate"]}, {"failed": ref["failed"], "d_lambda": ref["rate"], "cancel_d_lambda": ref["cancel_rate"]},
                 C_BOUND, "cafe_branch_scores: " + label)


@pytest.mark.gpu
def test_the_gemm_launches_are_the_gradient_calls(capi):
    pb, pr, mus, _ = pair_case(64, 40, "gamma_err_rho_0.25", "max")
    ctx = capi.Context(pb, max_categories=TS._K(pr))
    try:
        ctx.set_death_rates(mus)
        ctx.score_gradient(pr, "max", alpha=0.7)
        _, want = ctx.marginal_gemm_stats()
        ctx.branch_scores(pr, "max", alpha=0.7)
        _, got = ctx.marginal_gemm_stats()
    finally:
        ctx.close()
    assert want > 0 and got == want


@pytest.mark.gpu
def test_null_outputs_the_dimension_and_the_state_error(capi):
    pb, pr, mus, ref = pair_case(16, 14, "gamma_err_rho_0.25", "sum")
    ctx = capi.Context(pb, max_categories=TS._K(pr))
    try:
        assert ctx.branch_scores_dim(pr) == (pb.n_nodes - 1) + pb.n_lambdas + 3
        with pytest.raises(capi.CafeError, match="death rates"):
            ctx.branch_scores(pr, "sum", alpha=0.7, death_rates=True)
        ctx.set_death_rates(mus)
        P_ = ctx.branch_scores_dim(pr)
        assert P_ == 2 * (pb.n_nodes - 1) + 2 * pb.n_lambdas + 3
        full = ctx.branch_scores(pr, "sum", alpha=0.7)
        only_gram = ctx.branch_scores(pr, "sum", alpha=0.7, per_family=False)
        only_rows = ctx.branch_scores(pr, "sum", alpha=0.7, gram=False)
    finally:
        ctx.close()
    assert full["gram"].shape == (P_, P_) and "rate" not in only_gram and "gram" not in only_rows
    for key in only_gram:
        assert np.array_equal(only_gram[key], full[key], equal_nan=True), key
    for key in only_rows:
        assert np.array_equal(only_rows[key], full[key], equal_nan=True), key


# ------------------------------------------------------------------------------------------------------ the kernel alone
def gram_case(p, n):
    rng = np.random.default_rng(1000 * p + n)
    S = rng.standard_normal((p, n)) * np.exp(rng.uniform(-6, 6, size=(p, 1)))
    w = rng.integers(0, 5, size=n).astype(float)             # zeros among them
    w[::3] += rng.uniform(0, 1, size=len(w[::3]))            # and non-integers
    if n > 4:
        w[1] = 0.0
    return S, w


@pytest.mark.gpu
@pytest.mark.parametrize("p", [1, 15, 16, 17, 33])
def test_the_weighted_gram_kernel_alone(capi, p):
    for n in [1, 3, 4, 5, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3]:
        S, w = gram_case(p, n)
        gram, total = capi.weighted_gram(S, w)
        again, total2 = capi.weighted_gram(S, w)
        assert np.array_equal(gram, again) and np.array_equal(total, total2), (p, n)
        assert np.array_equal(gram, gram.T), (p, n)
        L = S.astype(np.longdouble)                          # the reference in extended precision: its own error is not in the bound
        ref, room = (L * w) @ L.T, 2 * n * EPS * ((np.abs(L) * w) @ np.abs(L).T)
        assert np.all(np.abs(gram - ref) <= room), (p, n, np.max(np.abs(gram - ref)[room > 0] / room[room > 0]))
        assert np.all(np.abs(total - L @ w) <= 2 * n * EPS * (np.abs(L) @ w)), (p, n)


@pytest.mark.gpu
def test_a_zero_weight_hides_whatever_the_column_holds(capi):
    S, w = gram_case(17, 70)
    w[5] = w[69] = 0.0
    want = capi.weighted_gram(S, w)
    S[:, 5], S[3, 69] = np.nan, np.inf
    got = capi.weighted_gram(S, w)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
