"""cafe_score_gradient on the device against tests/gradient_ref.py and against the entry points the library already had.

Inputs: the six-taxon problem of tests/bd_lm_ref.py at orders 41 (M 40, R 30) and 300 (M 299, R 250) -- a cherry, a
trifurcation and a leaf under the root, two lambda classes -- base model, gamma K = 3 and a 3-tap error model, with
lambda = mu and with death rates set, under both root rules.

Against gradient_ref.reverse: |got - ref| <= 1e-12 + 1e-10 c |ref|.  1e-10 is the project's bound for sums without
cancellation (test_marginal_gpu.py); c = 1000 is the largest cancellation factor sum |terms| / |sum terms| the reference
reports on these inputs, rounded up to a power of ten (measured on the CPU: 742 at order 41, 512 at order 300, both for
the gamma model with death rates; test_the_reference_reports_the_cancellation_the_bound_assumes asserts it).
family_lnl: cafe_score's per-family value (MAX) and cafe_marginal_reconstruct's log_evidence (SUM) at those tests' own
bound, 1e-12 + 1e-10 |ref|.

Against the parent's functions: central differences of cafe_score's family results (MAX) and of log_evidence (SUM) with
h = 1e-4 lambda on quantized points, divided by the actual difference of the quantized rates; 1e-6 relative (truncation
(h / lambda)^2 = 1e-8 times a ratio of derivatives, measured 5e-9 on the CPU) plus the rounding of the quotient itself,
4 eps |lnL| / |difference|.  Under MAX a family whose arg max differs between the two points is left out, at most 5 % of
the families (the reference alone: tests/test_gradient_model.py)."""
import functools

import numpy as np
import pytest

import bd_lm_ref as BL
import gradient_ref as GR
from cafexp_amd import problem as P

C_BOUND = 1000.0
MODELS = ("base", "gamma", "error")
RATES = {"lambda_eq_mu": None, "death_rates": BL.MUS}


def _case(order, model):
    pb = BL.problem(order, n_dev=3 if model == "error" else 0)
    return pb, BL.params(pb, model)


@functools.lru_cache(maxsize=None)
def _reference(order, model, rates, rule):
    pb, pr = _case(order, model)
    return GR.reverse(pb, pr, RATES[rates], rule)


@pytest.mark.parametrize("order", [41, 300])
def test_the_reference_reports_the_cancellation_the_bound_assumes(order):
    worst = max(GR.worst_cancellation(_reference(order, m, r, rule)) for m in MODELS for r in RATES for rule in ("max", "sum"))
    print("order %d: largest cancellation factor %.1f" % (order, worst))
    assert C_BOUND / 10 < worst <= C_BOUND


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _within(g, r):
    return np.all(np.abs(g - r) <= 1e-12 + 1e-10 * np.abs(r))


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("order", [41, 300])
def test_matches_the_reference_and_the_shipped_values(capi, order, model):
    pb, pr = _case(order, model)
    K = 3 if model == "gamma" else 1
    ctx = capi.Context(pb, max_categories=K)
    try:
        for rates, mus in RATES.items():
            ctx.set_death_rates(mus)
            _, fam = ctx.score(pr, alpha=0.7, per_family=True)
            evidence = ctx.marginal_reconstruct(pr, alpha=0.7)["log_evidence"]
            for rule in ("max", "sum"):
                got = ctx.score_gradient(pr, rule, alpha=0.7)
                assert ("d_mu" in got) == (mus is not None) and ("d_multiplier" in got) == (model == "gamma")
                GR.close(got, _reference(order, model, rates, rule), C_BOUND, "order %d %s %s %s" % (order, model, rates, rule))
                assert _within(got["family_lnl"], fam["family_lnl"] if rule == "max" else evidence), (rates, rule)
    finally:
        ctx.close()


def _quotients(ctx, pr, mus, kind, q, value):
    lam0 = np.array(pr.lambdas, dtype=float)
    mu0 = None if mus is None else np.array(mus, dtype=float)
    h = 1e-4 * lam0[q]
    vals, pts = [], []
    for sign in (-1.0, 1.0):
        lam, mu = lam0.copy(), None if mu0 is None else mu0.copy()
        (lam if kind == "lambda" else mu)[q] += sign * h
        pts.append(BL.quantize((lam if kind == "lambda" else mu)[q], 0.0, 0.0)[0])
        ctx.set_death_rates(mu)
        vals.append(value(P.Params(lambdas=lam, prior=pr.prior, multipliers=pr.multipliers, cat_probs=pr.cat_probs, error_model=pr.error_model)))
    ctx.set_death_rates(mus)
    width = pts[1] - pts[0]
    return (vals[1] - vals[0]) / width, 4 * np.finfo(float).eps * np.abs(vals[0]) / width, pts


@pytest.mark.gpu
@pytest.mark.parametrize("rates", sorted(RATES))
@pytest.mark.parametrize("model", ["base", "error"])
def test_central_differences_of_the_shipped_entry_points(capi, model, rates):
    order = 41
    pb, pr = _case(order, model)
    mus = RATES[rates]
    ctx = capi.Context(pb)
    try:
        ctx.set_death_rates(mus)
        grads = {rule: ctx.score_gradient(pr, rule) for rule in ("max", "sum")}
        values = {"max": lambda p: ctx.score(p, per_family=True)[1]["family_lnl"], "sum": lambda p: ctx.marginal_reconstruct(p)["log_evidence"]}
        for rule in ("max", "sum"):
            for kind in ["lambda"] + ([] if mus is None else ["mu"]):
                for q in range(pb.n_lambdas):
                    fd, floor, pts = _quotients(ctx, pr, mus, kind, q, values[rule])
                    keep = np.ones(pb.n_families, dtype=bool)
                    if rule == "max":                        # the arg max at the two points, from the reference's prune
                        args = []
                        for x in pts:
                            lam, mu = np.array(pr.lambdas, dtype=float), None if mus is None else np.array(mus, dtype=float)
                            (lam if kind == "lambda" else mu)[q] = x
                            a = []
                            GR.log_z(pb, P.Params(lambdas=lam, prior=pr.prior, error_model=pr.error_model), mu, "max", args=a)
                            args.append(a[0])
                        keep = args[0] == args[1]
                        assert (~keep).sum() <= 0.05 * pb.n_families
                    g = grads[rule]["d_" + kind][:, q]
                    err, bound = np.abs(fd - g)[keep], (1e-6 * np.abs(g) + floor)[keep]
                    print("%s %s %s d_%s[%d]: worst |fd - g| / bound %.3g" % (model, rates, rule, kind, q, (err / bound).max()))
                    assert np.all(err <= bound), (rule, kind, q)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_arguments_and_states(capi):
    pb, pr = _case(41, "base")
    ctx = capi.Context(pb)
    try:
        with pytest.raises(capi.CafeError, match="code 4"):           # d_mu without death rates: CAFE_ERR_STATE
            ctx.score_gradient(pr, "max", death_rates=True)
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.score_gradient(pr, 7)
        bad = P.Params(lambdas=np.array([-0.01, 0.006]), prior=pr.prior)
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.score_gradient(bad, "max")
        gm = BL.params(pb, "gamma")                                   # K = 3 on a context made for one category
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.score_gradient(gm, "max")
        before = ctx.score(pr)
        ctx.score_gradient(pr, "sum")
        assert ctx.score(pr) == before                                # a later cafe_score is unaffected
    finally:
        ctx.close()
