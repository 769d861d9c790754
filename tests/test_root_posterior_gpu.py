"""cafe_root_posterior on the device: against the root node's row of cafe_marginal_reconstruct (mean, mode, log_evidence) and
against tests/root_rule_ref.py fed the matrices the call itself built (total, n_used, category_posterior).

Inputs and bound as tests/test_root_rule_gpu.py: |got - ref| <= 1e-12 + 1e-10 |ref|; total additionally with an absolute
floor of 1e-12 n_families (it is a sum over the families).  mode: exact -- the reference has no two best masses within 1e-9
on these inputs (tests/test_root_rule_model.py)."""
import ctypes

import numpy as np
import pytest

import marginal_ref as MR
import root_rule_ref as RR
from cafexp_amd import problem as P
from test_gradient_shapes import _saturated_case
from test_root_rule_gpu import capi, reference, same_bits, within  # noqa: F401 (capi: the fixture)
from test_root_rule_model import MODELS, ORDERS, RATES, REPS, case

pytestmark = pytest.mark.gpu


def within_total(got, ref, n_families, label):
    d = np.abs(np.asarray(got) - np.asarray(ref))
    lim = np.maximum(RR.bound(ref), 1e-12 * n_families)
    print("%s: worst |d| / bound = %.3g" % (label, float(np.max(d / lim))))
    assert np.all(d <= lim), label


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("order", ORDERS)
def test_matches_the_marginal_reconstruction_and_the_reference(capi, order, model):
    pb, pr = case(order, model)
    K = 3 if model == "gamma" else 1
    root = MR.root_of(pb)
    ctx = capi.Context(pb, max_categories=K)
    try:
        for rates, mus in RATES.items():
            label = "order %d %s %s" % (order, model, rates)
            ctx.set_death_rates(mus)
            got = ctx.root_posterior(pr, alpha=0.7)
            ref = RR.root_posterior(pr, reference(ctx, pb, pr, K))
            marg = ctx.marginal_reconstruct(pr, alpha=0.7)
            assert not got["failed"].any() and got["n_used"] == ref["n_used"] == len(REPS)
            within(got["mean"], marg["mean"][:, root], label + " mean against the root's row")
            assert np.array_equal(got["mode"], marg["mode"][:, root]) and np.array_equal(got["mode"], ref["mode"])
            within(got["log_evidence"], marg["log_evidence"], label + " log_evidence against the marginal call")
            within(got["mean"], ref["mean"], label + " mean against numpy")
            within(got["log_evidence"], ref["log_evidence"], label + " log_evidence against numpy")
            within_total(got["total"], ref["total"], pb.n_families, label + " total")
            within_total(got["total"].sum(), got["n_used"], pb.n_families, label + " sum of total against n_used")
            if model == "gamma":
                within(got["category_posterior"], ref["category_posterior"], label + " category_posterior")
            else:
                assert "category_posterior" not in got
            ctx.set_root_rule("sum")                         # the scorer's own bits under the sum rule
            _, fam = ctx.score(pr, alpha=0.7, per_family=True)
            ctx.set_root_rule("max")
            assert same_bits(fam["family_lnl"], got["log_evidence"]), label
            assert np.array_equal(got["mean"][8:], got["mean"][REPS[8:]])
    finally:
        ctx.close()


def test_a_failed_family_is_left_out(capi):
    """Half of the families are impossible under a saturated branch (test_gradient_shapes.py's case): NaN doubles, mode -1,
    failed = 1, nothing added to total."""
    pb, pr, possible = _saturated_case()
    ctx = capi.Context(pb)
    try:
        got = ctx.root_posterior(pr)
        mats = MR.context_matrices(ctx, pb, 1)
        ref = RR.root_posterior(pr, RR.root_vectors(pb, pr, mats))
        assert np.array_equal(got["failed"] == 0, possible) and np.array_equal(got["failed"], ref["failed"])
        assert got["n_used"] == int(possible.sum()) == ref["n_used"]
        assert np.all(np.isnan(got["mean"][~possible])) and np.all(np.isnan(got["log_evidence"][~possible]))
        assert np.all(got["mode"][~possible] == -1) and np.array_equal(got["mode"], ref["mode"])
        within(got["mean"][possible], ref["mean"][possible], "saturated mean")
        within_total(got["total"], ref["total"], pb.n_families, "saturated total")
        within_total(got["total"].sum(), got["n_used"], pb.n_families, "saturated sum of total")
    finally:
        ctx.close()


def test_errors_and_the_scorer_afterwards(capi):
    pb, pr = case(41, "base")
    gpb, gpr = case(41, "gamma")
    ctx = capi.Context(pb)                                   # made for one category
    try:
        before = ctx.score(pr, per_family=True)
        with pytest.raises(capi.CafeError, match="code 1"):  # bad K
            ctx.root_posterior(gpr, alpha=0.7)
        with pytest.raises(capi.CafeError, match="code 1"):  # invalid rate
            ctx.root_posterior(P.Params(lambdas=np.array([-0.01, 0.006]), prior=pr.prior))
        ro = capi.CafeRootPosteriorOut()                     # category_posterior under the base model
        buf = np.empty((pb.n_families, 1))
        ro.category_posterior = capi._p(buf, capi._f64p)
        cp, keep = ctx._params(pr)
        assert ctx._lib.cafe_root_posterior(ctx._h, ctypes.byref(cp), ctypes.byref(ro)) == 1
        assert b"gamma" in ctx._lib.cafe_last_error(ctx._h)
        ctx.comm_attach(capi.comm_unique_id(), 1, 0)         # a communicator of one rank
        with pytest.raises(capi.CafeError, match="code 4"):
            ctx.root_posterior(pr)
        ctx.comm_detach()
        ctx.root_posterior(pr)
        with pytest.raises(capi.CafeError, match="code 4"):  # family results are not meaningful after the call
            ctx.family_results()
        after = ctx.score(pr, per_family=True)
        assert same_bits(before[0], after[0])
        for key in before[1]:
            assert np.array_equal(before[1][key], after[1][key]), key
    finally:
        ctx.close()
