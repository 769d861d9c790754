"""cafe_set_root_rule on the device: the scorer under CAFE_ROOT_SUM against tests/root_rule_ref.py fed the matrices the call
itself built (Context.matrix: K1's pinned parity is not tested again) and against cafe_marginal_reconstruct's log_evidence;
the max rule bit for bit what it is without the setter.

Inputs: tests/test_root_rule_model.py's -- the six-taxon problem of tests/bd_lm_ref.py at orders 41 and 300 with repeated
families and a prior ~ 1 / s; base model, gamma K = 3, a 3-tap error model; lambda = mu and death rates.  Every comparison
of doubles: |got - ref| <= 1e-12 + 1e-10 |ref|, the project's bound for sums without cancellation (test_marginal_gpu.py)."""
import numpy as np
import pytest

import marginal_ref as MR
import root_rule_ref as RR
from cafexp_amd import problem as P
from test_gradient_shapes import _saturated_case
from test_root_rule_model import DISTINCT, MODELS, ORDERS, RATES, REPS, case, underflow_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def within(got, ref, label):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref)
    d = np.where(got == ref, 0.0, d)                         # (equal infinities)
    worst = float(np.max(d / RR.bound(ref))) if d.size else 0.0
    print("%s: worst |d| / bound = %.3g" % (label, worst))
    assert np.all(d <= RR.bound(ref)), (label, worst)


def reference(ctx, pb, pr, K):
    """root vectors of every family from the matrices of the context's last call"""
    mats = MR.context_matrices(ctx, pb, K)
    return RR.root_vectors(pb, pr, mats, families=list(DISTINCT))[REPS]


def per_family(ctx, pb, pr, mus):
    fams = np.arange(pb.n_families)
    lam = np.tile(pr.lambdas, (pb.n_families, 1))
    if mus is None:
        return ctx.score_per_family(pr, fams, lam)
    return ctx.score_per_family_lm(pr, fams, lam, np.tile(mus, (pb.n_families, 1)))


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("order", ORDERS)
def test_the_sum_rule_matches_the_reference_and_the_log_evidence(capi, order, model):
    pb, pr = case(order, model)
    K = 3 if model == "gamma" else 1
    ctx = capi.Context(pb, max_categories=K)
    try:
        for rates, mus in RATES.items():
            label = "order %d %s %s" % (order, model, rates)
            ctx.set_death_rates(mus)
            ctx.set_root_rule("max")
            _, fam_max = ctx.score(pr, alpha=0.7, per_family=True)
            ctx.set_root_rule("sum")
            assert ctx.root_rule() == "sum"
            value, fam = ctx.score(pr, alpha=0.7, per_family=True)
            ref = RR.sum_rule(pr, reference(ctx, pb, pr, K))
            within(fam["family_lnl"], ref["family_lnl"], label + " family_lnl against numpy")
            within(value, -np.sum(fam["family_lnl"]), label + " -lnL against the sum of its families")
            within(value, RR.neg_lnl(ref["family_lnl"]), label + " -lnL against numpy")
            assert np.array_equal(fam["failed"], fam_max["failed"]) and np.all(fam["family_lnl"] >= fam_max["family_lnl"])
            if model == "gamma":
                within(fam["category_likelihood"], ref["category_likelihood"], label + " category_likelihood")
                within(fam["family_likelihood"], ref["family_likelihood"], label + " family_likelihood")
            else:
                within(per_family(ctx, pb, pr, mus), fam["family_lnl"], label + " per-family entry against cafe_score")
            evidence = ctx.marginal_reconstruct(pr, alpha=0.7)["log_evidence"]
            within(fam["family_lnl"], evidence, label + " family_lnl against log_evidence")
    finally:
        ctx.close()


def _everything(ctx, pb, pr, mus, with_per_family):
    value, fam = ctx.score(pr, alpha=0.7, per_family=True)
    out = [np.float64(value)] + [fam[k] for k in sorted(fam)]
    if with_per_family:
        out.append(per_family(ctx, pb, pr, mus))
    return out


@pytest.mark.parametrize("model", MODELS)
def test_the_max_rule_keeps_its_bits(capi, model):
    """A context that went to the sum rule and back, and a fresh one, against values recorded before the setter was ever
    called; then, with graphs on, the rules alternating: each gives the bits of its stream path."""
    pb, pr = case(41, model)
    K = 3 if model == "gamma" else 1
    for mus in RATES.values():
        a, b = capi.Context(pb, max_categories=K), capi.Context(pb, max_categories=K)
        try:
            a.set_death_rates(mus)
            b.set_death_rates(mus)
            recorded = _everything(a, pb, pr, mus, model != "gamma")
            a.set_root_rule("sum")
            summed = _everything(a, pb, pr, mus, model != "gamma")
            assert summed[0] < recorded[0]                   # (-lnL: the sum is above its largest term)
            a.set_root_rule("max")
            for ctx in (a, b):
                again = _everything(ctx, pb, pr, mus, model != "gamma")
                assert len(again) == len(recorded) and all(same_bits(x, y) for x, y in zip(again, recorded))
            a.set_graphs(True)
            for rule, want in (("max", recorded), ("sum", summed), ("max", recorded), ("sum", summed), ("sum", summed), ("max", recorded)):
                a.set_root_rule(rule)
                got = _everything(a, pb, pr, mus, False)
                assert all(same_bits(x, y) for x, y in zip(got, want)), rule
            with pytest.raises(capi.CafeError, match="code 1"):
                a.set_root_rule(2)
            assert a.root_rule() == "max"
        finally:
            a.close()
            b.close()


def test_underflow_keeps_a_finite_value(capi):
    """Every L_j prior_j of the first family underflows a double (asserted on the CPU, test_root_rule_model.py): the base
    model's log-sum-exp returns the reference's finite value where log_evidence reports a failure."""
    pb, pr = underflow_case()
    ctx = capi.Context(pb)
    try:
        ctx.set_root_rule("sum")
        value, fam = ctx.score(pr, per_family=True)
        mats = MR.context_matrices(ctx, pb, 1)
        ref = RR.sum_rule(pr, RR.root_vectors(pb, pr, mats))["family_lnl"]
        assert np.isfinite(ref).all() and ref[0] < -745.0
        within(fam["family_lnl"], ref, "underflow family_lnl")
        within(value, -ref.sum(), "underflow -lnL")
        marg = ctx.marginal_reconstruct(pr)
        assert list(marg["failed"]) == [1, 0] and np.isnan(marg["log_evidence"][0])
        post = ctx.root_posterior(pr)
        assert list(post["failed"]) == [1, 0] and post["n_used"] == 1
    finally:
        ctx.close()


@pytest.mark.parametrize("model", ["base", "gamma"])
def test_an_empty_prior_support_is_minus_infinity(capi, model):
    """A prior that is zero wherever a family's root vector is not: -inf per family, +inf for the call, never NaN.  First a
    prior of zeros for every family; then the families a saturated branch makes impossible (L = 0 at every root size)."""
    pb, pr = case(41, model)
    K = 3 if model == "gamma" else 1
    ctx = capi.Context(pb, max_categories=K)
    try:
        ctx.set_root_rule("sum")
        pr.prior = np.zeros(pb.max_root_family_size, dtype=np.float32)
        value, fam = ctx.score(pr, alpha=0.7, per_family=True)
        assert value == np.inf and np.all(fam["family_lnl"] == -np.inf)
        pr.prior[3] = 1.0
        value, fam = ctx.score(pr, alpha=0.7, per_family=True)
        assert np.isfinite(value) and np.isfinite(fam["family_lnl"]).all()
    finally:
        ctx.close()
    if model == "gamma":
        return
    pb, pr, possible = _saturated_case()
    ctx = capi.Context(pb)
    try:
        ctx.set_root_rule("sum")
        value, fam = ctx.score(pr, per_family=True)
        assert value == np.inf
        assert np.all(fam["family_lnl"][~possible] == -np.inf) and np.isfinite(fam["family_lnl"][possible]).all()
        pf = ctx.score_per_family(pr, np.arange(pb.n_families), np.tile(pr.lambdas, (pb.n_families, 1)))
        assert np.all(pf[~possible] == -np.inf)
        within(pf[possible], fam["family_lnl"][possible], "saturated: per-family entry against cafe_score")
    finally:
        ctx.close()
