"""cafe_leaf_predictive on the device, on the shipped examples, against tests/leaf_predictive_ref.py fed the matrices the call
itself built (Context.matrix), so that K1's pinned parity is not tested again.

The mammals example (its first 24 families) under the base model, under gamma K = 4 and with an error model; a two-lambda tree
with the class of one leaf at 0, whose branch carries a key that is marked zero: its matrix is what K1 built for such a key, the
call makes no special case of it, and cells are finite or NaN exactly where the reference's are.  (With the class of the mammals'
chimp / human lambda tree at 0 an interior branch is frozen too, every family is impossible and the few cells with mass have it
in the subnormal range: not a case that can be held to a relative bound.)  Bound: |got - ref| <= 1e-12 + 1e-10 c |ref|,
sd held to its own 1 + (mean - x)^2 / var capped at test_leaf_predictive_shapes.C_BOUND, everything else to c = 1.

The call leaves a following cafe_score as one made before it, and refuses what the other posterior calls refuse, with their
codes and texts."""
import dataclasses

import numpy as np
import pytest

import leaf_predictive_ref as LR
import marginal_ref as MR
from cafexp_amd import problem as P
from cafexp_amd.gamma_rates import discrete_gamma
from helpers import case_from_args
from oracle import oracle as O
from test_gradient_shapes import _saturated_case
from test_leaf_predictive_shapes import C_BOUND
from test_per_family_shapes import THREE_TAPS

pytestmark = pytest.mark.gpu

MAMMALS = {"tree": "mammals_tree.txt", "families": "mammal_gene_families.txt"}
CASES = {
    "mammals_base": dict(MAMMALS, limit=24, **{"lambda": 0.0018}),
    "mammals_gamma_k4": dict(MAMMALS, limit=24, model="gamma", k=4, alpha=0.425, **{"lambda": 0.002}),
    "mammals_error_model": dict(MAMMALS, limit=24, errfile="errormodel_0.1.txt", **{"lambda": 0.0018}),
}
ARGUMENT, STATE = 1, 4                                       # CAFE_ERR_ARGUMENT, CAFE_ERR_STATE


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _K(pr):
    return 1 if pr.multipliers is None else len(pr.multipliers)


def _run(capi, name):
    pb, pr, alpha = case_from_args(CASES[name], O)
    ctx = capi.Context(pb, max_categories=_K(pr))
    try:
        got = ctx.leaf_predictive(pr, alpha=alpha)
        ref = LR.reference(pb, pr, MR.context_matrices(ctx, pb, _K(pr)))
    finally:
        ctx.close()
    return pb, got, ref


@pytest.mark.parametrize("name", ["mammals_base", "mammals_gamma_k4", "mammals_error_model"])
def test_the_mammals_example(capi, name):
    pb, got, ref = _run(capi, name)
    LR.close(got, ref, C_BOUND, name)
    assert not got["failed"].any() and not np.isnan(got["mean"]).any()
    assert np.all(np.abs(got["p_below"] + got["p_obs"] + got["p_above"] - 1.0) <= 1e-12)
    assert np.all(got["sd"] > 0) and np.all(got["p_obs"] > 0)


def test_a_lambda_class_at_zero(capi):
    """The three-taxon problem of test_gradient_shapes' saturated case with the lambda class of leaf A at 0: the key of A's
    branch is marked zero, its matrix is e_0 in row 0 and zero below.  Families with A = B = 0 are possible; in the others some
    cells have no mass (NaN) and some are finite with p_obs = 0 -- the observation is impossible, its prediction is not."""
    pb, pr, possible = _saturated_case()
    pb.counts[1, :2] = [3, 0]
    possible[1] = False
    pr = P.Params(lambdas=np.array([0.02, 0.0]), prior=pr.prior)
    mats = LR.matrices(pb, pr)
    assert np.count_nonzero(mats[0][int(np.where(pb.lambda_index == 1)[0][0])]) == 1
    ref = LR.reference(pb, pr, mats)
    W = ref["W"]
    assert W[W > 0].min() > 1e-250 and (W == 0).any() and np.array_equal(ref["failed"] == 0, possible)
    assert np.isnan(ref["mean"]).any() and (ref["p_obs"] == 0).any() and not np.isnan(ref["mean"][possible]).any()
    ctx = capi.Context(pb)
    try:
        got = ctx.leaf_predictive(pr)
        LR.close(got, LR.reference(pb, pr, MR.context_matrices(ctx, pb, 1)), C_BOUND, "one class at zero, the call's matrices")
    finally:
        ctx.close()
    LR.close(got, ref, C_BOUND, "one class at zero")          # the same NaN pattern, the same failed families
    assert np.array_equal(got["p_obs"] == 0, ref["p_obs"] == 0)


def test_a_following_score_is_the_one_made_before(capi):
    pb, pr, alpha = case_from_args(CASES["mammals_gamma_k4"], O)
    ctx = capi.Context(pb, max_categories=_K(pr))
    try:
        before = ctx.score(pr, alpha=alpha, per_family=True)
        ctx.leaf_predictive(pr, alpha=alpha)
        after = ctx.score(pr, alpha=alpha, per_family=True)
    finally:
        ctx.close()
    assert after[0] == before[0]
    for key in before[1]:
        assert np.array_equal(after[1][key], before[1][key], equal_nan=True), key


def test_the_gemm_launches_are_reported(capi):
    """cafe_debug_marginal_gemm: the up pass and one kDown launch per interior branch -- two thirds of what
    cafe_marginal_reconstruct reports, which adds two half-run split launches -- and the new GEMM per leaf branch, all columns"""
    pb, pr, alpha = case_from_args(CASES["mammals_base"], O)
    ctx = capi.Context(pb)
    try:
        ctx.leaf_predictive(pr)
        _, flops = ctx.marginal_gemm_stats()
        ctx.marginal_reconstruct(pr)
        _, marginal = ctx.marginal_gemm_stats()
    finally:
        ctx.close()
    M, R = pb.max_family_size, pb.max_root_family_size
    root = MR.root_of(pb)
    size = lambda v: R if pb.parent[v] == root else M        # sizes 1..size(v) of v's parent
    interior = sum(2.0 * (M + 1) * size(v) for v in range(pb.n_nodes) if v != root and pb.leaf_taxon[v] < 0)
    leaves = sum(2.0 * (M + 1) * (size(v) + 1) for v in range(pb.n_nodes) if pb.leaf_taxon[v] >= 0)
    columns = marginal / (3 * interior)
    assert columns >= 128 and columns % 128 == 0
    assert flops == (2 * interior + leaves) * columns


def test_the_refusals_of_the_posterior_calls(capi):
    pb, pr, alpha = case_from_args(CASES["mammals_base"], O)
    ctx = capi.Context(pb)                                   # one category, no error model
    try:
        probs, mult = discrete_gamma(3, 0.7)
        cases = [
            (dataclasses.replace(pr, multipliers=mult, cat_probs=probs), ARGUMENT,
             "cafe_leaf_predictive: gamma model needs 1..1 categories with multipliers and cat_probs"),
            (dataclasses.replace(pr, lambdas=np.array([-0.01])), ARGUMENT, "cafe_leaf_predictive: invalid lambda or death rate"),
            (dataclasses.replace(pr, error_model=P.error_model_table(THREE_TAPS, pb.max_family_size)), ARGUMENT,
             "cafe_leaf_predictive: the context was created without an error model"),
        ]
        fresh = ctx.leaf_predictive(pr)
        for bad, code, text in cases:
            with pytest.raises(capi.CafeError) as e:
                ctx.leaf_predictive(bad)
            assert str(e.value) == "code %d: %s" % (code, text)
            again = ctx.leaf_predictive(pr)                  # a refused call leaves no trace
            for key in fresh:
                assert np.array_equal(again[key], fresh[key], equal_nan=True), key
        ctx.comm_attach(capi.comm_unique_id(), 1, 0)
        with pytest.raises(capi.CafeError) as e:
            ctx.leaf_predictive(pr)
        assert str(e.value) == "code %d: cafe_leaf_predictive: not valid on a context with a communicator attached" % STATE
        ctx.comm_detach()
        import ctypes as C
        cp, keep = ctx._params(pr)
        assert ctx._lib.cafe_leaf_predictive(ctx._h, C.byref(cp), None) == ARGUMENT
        assert ctx._lib.cafe_last_error(ctx._h).decode() == "cafe_leaf_predictive: lambdas, prior and out are required"
    finally:
        ctx.close()
