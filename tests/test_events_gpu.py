"""cafe_expected_events on the device against tests/events_ref.py and against the entry points the library already had.

Inputs: the 13-taxon problem of tests/test_gradient_shapes.py at M = 40, R = 30 -- a cherry, a polytomy of 7 leaves, a clade with
an interior child, a leaf under the root, two lambda classes, 24 families with counts 0 and M at leaves (under the 3-tap error
model those taps fall outside [0, M]) and duplicates -- in CONFIGS: base and gamma K = 2, lambda = mu and death rates at
rho = mu / lambda of 0.25 and 4, with and without the error model.  The saturated three-taxon problem of the same file: one
branch whose key is marked zero, and every other family impossible (Z = 0).

Against events_ref.reference (the complex-step rows): |got - ref| <= 1e-12 + 1e-10 c |ref|, the gradient's rule, with c = 1: the
six coefficients are non-negative, so every entry is a sum of non-negative terms and the reference reports no cancellation
(test_the_reference_reports_no_cancellation asserts it).

Against the parent's calls, where differences do cancel, every entry is held to 1e-10 of the sum of the |terms| behind it:
  gains - losses on the branch above v  =  mean[v] - mean[parent(v)] of cafe_marginal_reconstruct
      (bound 1e-12 + 1e-10 (gains + losses + mean[v] + mean[parent]));
  death rates equal to the lambdas:  lambda_q (d_lambda - d_mu)[q] of cafe_score_gradient(CAFE_ROOT_SUM)  =  sum_{v in q} (gains -
      losses)  (bound 1e-12 + 1e-10 (lambda_q (c_l |d_lambda| + c_m |d_mu|) + sum (gains + losses)), c_l and c_m the
      cancellation factors gradient_ref.reverse reports for the two partials)."""
import functools

import numpy as np
import pytest

import events_ref as ER
import gradient_ref as GR
import marginal_ref as MR
from cafexp_amd import problem as P
from cafexp_amd.gamma_rates import discrete_gamma
from test_gradient_shapes import LAMBDAS, _problem, _prior, _saturated_case
from test_per_family_shapes import THREE_TAPS

C_BOUND = 1.0
CONFIGS = {
    "base": dict(K=1, err=False, mus=None),
    "base_rho_0.25": dict(K=1, err=False, mus=LAMBDAS * 0.25),
    "base_err_rho_4": dict(K=1, err=True, mus=LAMBDAS * 4),
    "gamma2": dict(K=2, err=False, mus=None),
    "gamma2_err_rho_0.25": dict(K=2, err=True, mus=LAMBDAS * 0.25),
}


def _params(pb, cfg):
    pr = P.Params(lambdas=LAMBDAS.copy(), prior=_prior(pb.max_root_family_size))
    if cfg["K"] > 1:
        pr.cat_probs, pr.multipliers = discrete_gamma(cfg["K"], 0.7)
    if cfg["err"]:
        pr.error_model = P.error_model_table(THREE_TAPS, pb.max_family_size)
    return pr


@functools.lru_cache(maxsize=None)
def _case(config):
    cfg = CONFIGS[config]
    pb = _problem(40, 30, err=cfg["err"])
    pr = _params(pb, cfg)
    return pb, pr, cfg["mus"], ER.reference(pb, pr, cfg["mus"], route="rows")


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_reference_reports_no_cancellation(config):
    pb, pr, mus, ref = _case(config)
    assert not ref["failed"].any()
    fl = ER.reference(pb, pr, mus, route="filters")
    assert ER.worst_cancellation(fl) <= C_BOUND + 1e-12
    ER.close(fl, ref, C_BOUND, "filters against rows, " + config)
    ok = ~np.isnan(ref["gains"])
    assert ref["gains"][ok].min() >= 0.0 and ref["losses"][ok].min() >= 0.0 and ref["gains"][ok].max() > 0.01


def test_turnover_is_visible_where_the_net_change_is_not():
    """what the call is for: on some branch gains and losses are both far above their difference"""
    ref = _case("base")[3]
    g, l = ref["gains"], ref["losses"]
    ok = ~np.isnan(g)
    assert np.any((np.minimum(g, l)[ok] > 10 * np.abs(g - l)[ok]) & (np.minimum(g, l)[ok] > 1e-3))


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _run(capi, pb, pr, mus, **ctx_args):
    ctx = capi.Context(pb, max_categories=1 if pr.multipliers is None else len(pr.multipliers), **ctx_args)
    try:
        ctx.set_death_rates(mus)
        return ctx.expected_events(pr, alpha=0.7)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_matches_the_reference(capi, config):
    pb, pr, mus, ref = _case(config)
    got = _run(capi, pb, pr, mus)
    ER.close(got, ref, C_BOUND, config)
    assert not got["failed"].any()
    root = MR.root_of(pb)
    for key in ER.KEYS:
        assert np.all(np.isnan(got[key][:, root])) and np.all(np.delete(got[key], root, axis=1) >= 0.0), key
        assert np.array_equal(got[key][4], got[key][2], equal_nan=True) and np.array_equal(got[key][5], got[key][0], equal_nan=True), key


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["base", "gamma2_err_rho_0.25", "base_err_rho_4"])
def test_gains_minus_losses_is_the_change_of_the_posterior_means(capi, config):
    pb, pr, mus, _ = _case(config)
    ctx = capi.Context(pb, max_categories=CONFIGS[config]["K"])
    try:
        ctx.set_death_rates(mus)
        ev = ctx.expected_events(pr, alpha=0.7)
        mr = ctx.marginal_reconstruct(pr, alpha=0.7)
    finally:
        ctx.close()
    assert np.all(np.abs(ev["log_evidence"] - mr["log_evidence"]) <= 1e-12 + 1e-10 * np.abs(mr["log_evidence"]))
    worst = 0.0
    for v in range(pb.n_nodes):
        p = int(pb.parent[v])
        if p < 0:
            continue
        net, change = ev["gains"][:, v] - ev["losses"][:, v], mr["mean"][:, v] - mr["mean"][:, p]
        bound = 1e-12 + 1e-10 * (ev["gains"][:, v] + ev["losses"][:, v] + mr["mean"][:, v] + mr["mean"][:, p])
        worst = max(worst, float(np.max(np.abs(net - change) / bound)))
    print("%s: worst |gains - losses - change of means| / bound %.3g" % (config, worst))
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2])
def test_equal_death_rates(capi, K):
    """mus == lambdas builds the lambda = mu matrices bit for bit (cafe_bd_rates) and the same coefficients: the unset call's
    bits; and the net events of a lambda class are lambda_q (d_lambda - d_mu) of the sum-rule score.  The second holds where
    the call's lambda_q IS the rate of the key, the base model with lambdas on the key's 1e-9 grid: the gamma model's keys are
    lambda_q m_k quantized, 1e-9 / lambda ~ 1e-7 away in relative terms from the factor the identity multiplies by, and the
    gradient's outputs are summed over the categories, so there it is not a statement about these outputs."""
    cfg = dict(K=K, err=True, mus=None)
    pb = _problem(40, 30, err=True)
    pr = _params(pb, cfg)
    ctx = capi.Context(pb, max_categories=K)
    try:
        unset = ctx.expected_events(pr, alpha=0.7)
        ctx.set_death_rates(LAMBDAS)
        both = ctx.expected_events(pr, alpha=0.7)
        grad = ctx.score_gradient(pr, "sum", alpha=0.7)
    finally:
        ctx.close()
    for key in unset:
        assert np.array_equal(both[key], unset[key], equal_nan=True), key
    if K > 1:
        return
    assert all(int(x * 1000000000) / 1000000000.0 == x for x in LAMBDAS)
    rv = GR.reverse(pb, pr, LAMBDAS, "sum")
    for q in range(pb.n_lambdas):
        nodes = [v for v in range(pb.n_nodes) if pb.parent[v] >= 0 and pb.lambda_index[v] == q]
        net = (both["gains"][:, nodes] - both["losses"][:, nodes]).sum(axis=1)
        lhs = LAMBDAS[q] * (grad["d_lambda"][:, q] - grad["d_mu"][:, q])
        room = LAMBDAS[q] * (rv["cancel_d_lambda"][:, q] * np.abs(rv["d_lambda"][:, q]) + rv["cancel_d_mu"][:, q] * np.abs(rv["d_mu"][:, q])) \
            + (both["gains"][:, nodes] + both["losses"][:, nodes]).sum(axis=1)
        print("K %d class %d: worst |lambda (d_lambda - d_mu) - net| / bound %.3g" % (K, q, np.max(np.abs(lhs - net) / (1e-12 + 1e-10 * room))))
        assert np.all(np.abs(lhs - net) <= 1e-12 + 1e-10 * room), q


@pytest.mark.gpu
def test_a_saturated_branch_has_no_events_and_an_impossible_family_fails(capi):
    pb, pr, possible = _saturated_case()
    ref = ER.reference(pb, pr, None, route="rows")
    assert np.array_equal(ref["failed"] == 0, possible)
    got = _run(capi, pb, pr, None)
    ER.close(got, ref, C_BOUND, "saturated")
    a = [v for v in range(pb.n_nodes) if pb.lambda_index[v] == 1 and pb.parent[v] >= 0]
    assert len(a) == 1
    others = [v for v in range(pb.n_nodes) if pb.parent[v] >= 0 and v != a[0]]
    assert np.array_equal(got["failed"] == 0, possible)
    for key in ER.KEYS:
        assert np.all(got[key][possible][:, a[0]] == 0.0) and np.all(got[key][possible][:, others].sum(axis=1) > 0.0), key
        assert np.all(np.isnan(got[key][~possible]))
    assert np.all(np.isnan(got["log_evidence"][~possible])) and np.all(np.isfinite(got["log_evidence"][possible]))
