"""The argument checks of the three posterior calls -- cafe_marginal_reconstruct, cafe_sample_histories, cafe_score_gradient --
are written once (sum_product.h) and take the entry's name.  Every refusal is pinned here by its code AND the full text of
cafe_last_error, the texts copied from the sources as they stood while each call carried its own copy of the checks; so is
the order in which the checks win when two arguments are wrong at once: communicator and required pointers, the call's own
range check, gamma categories, rates, error model, and for the gradient d_mu last.  The calls are made through the ctypes
handle, since the Python wrapper cannot express a missing prior.  After every refused call a valid call on the same context
returns, bit for bit, what a fresh context returns.

The three-taxon table of test_per_family_shapes at order 17, one context created with a 3-tap error model and one without,
both for at most two gamma categories."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from cafexp_amd import problem as P
from cafexp_amd.gamma_rates import discrete_gamma
from helpers import _explicit_problem
from test_per_family_shapes import THREE_TAPS, TREE3, families, sizes

ARGUMENT, STATE = 1, 4                                       # CAFE_ERR_ARGUMENT, CAFE_ERR_STATE
N, KMAX = 17, 2
CALLS = ("marginal", "history", "gradient")
EXPECTED = {
    ("marginal", "required"): (ARGUMENT, "cafe_marginal_reconstruct: lambdas, prior and out are required"),
    ("history", "required"): (ARGUMENT, "cafe_sample_histories: lambdas, prior and out are required"),
    ("gradient", "required"): (ARGUMENT, "cafe_score_gradient: lambdas, prior and out are required"),
    ("marginal", "categories"): (ARGUMENT, "cafe_marginal_reconstruct: gamma model needs 1..2 categories with multipliers and cat_probs"),
    ("history", "categories"): (ARGUMENT, "cafe_sample_histories: gamma model needs 1..2 categories with multipliers and cat_probs"),
    ("gradient", "categories"): (ARGUMENT, "cafe_score_gradient: gamma model needs 1..2 categories with multipliers and cat_probs"),
    ("marginal", "rate"): (ARGUMENT, "cafe_marginal_reconstruct: invalid lambda or death rate"),
    ("history", "rate"): (ARGUMENT, "cafe_sample_histories: invalid lambda or death rate"),
    ("gradient", "rate"): (ARGUMENT, "cafe_score_gradient: invalid lambda or death rate"),
    ("marginal", "error_model"): (ARGUMENT, "cafe_marginal_reconstruct: the context was created without an error model"),
    ("history", "error_model"): (ARGUMENT, "cafe_sample_histories: the context was created without an error model"),
    ("gradient", "error_model"): (ARGUMENT, "cafe_score_gradient: the context was created without an error model"),
    ("marginal", "own"): (ARGUMENT, "cafe_marginal_reconstruct: level must lie in (0, 1)"),
    ("history", "own"): (ARGUMENT, "cafe_sample_histories: n_draws must lie in 1..65536"),
    ("gradient", "own"): (ARGUMENT, "cafe_score_gradient: root_rule must be CAFE_ROOT_MAX or CAFE_ROOT_SUM"),
    ("gradient", "d_mu"): (STATE, "cafe_score_gradient: d_mu needs death rates (cafe_set_death_rates)"),
}
OWN_BAD = {"marginal": 1.5, "history": 0, "gradient": 7}     # level, n_draws, root_rule
OWN_GOOD = {"marginal": 0.9, "history": 3, "gradient": 0}
# case -> (the faults put into one call, the check that wins)
CASES = {
    "missing prior": (("required",), "required"),
    "too many categories": (("categories",), "categories"),
    "invalid rate": (("rate",), "rate"),
    "error model": (("error_model",), "error_model"),
    "own range check": (("own",), "own"),
    "d_mu without death rates": (("d_mu",), "d_mu"),
    "missing prior and own range": (("required", "own"), "required"),
    "own range and invalid rate": (("own", "rate"), "own"),
    "too many categories and invalid rate": (("categories", "rate"), "categories"),
    "invalid rate and error model": (("rate", "error_model"), "rate"),
    "invalid rate and d_mu": (("rate", "d_mu"), "rate"),
    "error model and d_mu": (("error_model", "d_mu"), "error_model"),
}


def _call(capi, ctx, call, pr, faults=(), alpha=1.0):
    """One call through the ctypes handle with `faults` put into otherwise valid arguments -> (code, cafe_last_error, outputs)"""
    lib, F, n, nl = ctx._lib, ctx.n_families, ctx.n_nodes, ctx.problem.n_lambdas
    if "rate" in faults:
        pr = dataclasses.replace(pr, lambdas=np.array([-0.01]))
    if "categories" in faults:
        pr = dataclasses.replace(pr)
        pr.cat_probs, pr.multipliers = discrete_gamma(KMAX + 1, 0.7)
    if "error_model" in faults:
        pr = dataclasses.replace(pr, error_model=P.error_model_table(THREE_TAPS, ctx.M))
    cp, keep = ctx._params(pr, alpha)
    if "required" in faults:
        cp.prior = None
    own = (OWN_BAD if "own" in faults else OWN_GOOD)[call]
    if call == "marginal":
        res = {"mean": np.empty((F, n)), "mode": np.empty((F, n), dtype=np.int32), "lo": np.empty((F, n), dtype=np.int32),
               "hi": np.empty((F, n), dtype=np.int32), "p_increase": np.empty((F, n)), "p_decrease": np.empty((F, n)),
               "log_evidence": np.empty(F), "failed": np.empty(F, dtype=np.int32)}
        out, fn, args = capi.CafeMarginalOut(), lib.cafe_marginal_reconstruct, (float(own),)
    elif call == "history":
        D = max(int(own), 1)
        res = {"sizes": np.empty((D, F, n), dtype=np.int32), "category": np.empty((D, F), dtype=np.int32), "n_increase": np.empty((D, n), dtype=np.int64),
               "n_decrease": np.empty((D, n), dtype=np.int64), "net_change": np.empty((D, n), dtype=np.int64), "log_evidence": np.empty(F),
               "failed": np.empty(F, dtype=np.int32)}
        out, fn, args = capi.CafeHistoryOut(), lib.cafe_sample_histories, (int(own), 20261019)
    else:
        res = {"family_lnl": np.empty(F), "d_lambda": np.empty((F, nl)), "failed": np.empty(F, dtype=np.int32)}
        if "d_mu" in faults:
            res["d_mu"] = np.empty((F, nl))
        if pr.multipliers is not None:
            res["d_multiplier"] = np.empty((F, len(pr.multipliers)))
        out, fn, args = capi.CafeGradientOut(), lib.cafe_score_gradient, (int(own),)
    for name, t in out._fields_:
        if name in res:
            setattr(out, name, res[name].ctypes.data_as(t))
    rc = fn(ctx._h, C.byref(cp), *args, C.byref(out))
    return rc, lib.cafe_last_error(ctx._h).decode(), res


@pytest.fixture(scope="module")
def setting():
    """capi, and per kind of context (its problem, valid parameters, alpha, what a fresh context returns for each call, the
    context the refused calls are made on)"""
    from cafexp_amd import capi
    capi.load()
    M, R = sizes(N)
    plain = _explicit_problem(TREE3, families(N), M, R)
    probs, mult = discrete_gamma(KMAX, 0.7)
    kinds = {
        "plain": (plain, P.Params(lambdas=np.array([0.01]), prior=P.prior_uniform(R)), 1.0),
        "error model": (dataclasses.replace(plain, n_deviations=3),
                        P.Params(lambdas=np.array([0.01]), prior=P.prior_uniform(R), multipliers=mult, cat_probs=probs,
                                 error_model=P.error_model_table(THREE_TAPS, M)), 0.7),
    }
    out = {}
    for kind, (pb, pr, alpha) in kinds.items():
        fresh = {}
        for call in CALLS:
            ctx = capi.Context(pb, max_categories=KMAX)
            rc, _, fresh[call] = _call(capi, ctx, call, pr, alpha=alpha)
            ctx.close()
            assert rc == 0, (kind, call)
            assert not fresh[call]["failed"].any(), (kind, call)
        out[kind] = (pr, alpha, fresh, capi.Context(pb, max_categories=KMAX))
    yield capi, out
    for _, _, _, ctx in out.values():
        ctx.close()


def test_the_problem_has_the_fields_the_setting_replaces():
    pb = _explicit_problem(TREE3, families(N), *sizes(N))
    assert pb.n_deviations == 0 and pb.n_lambdas == 1 and pb.matrix_size == N


# d_mu is an output of cafe_score_gradient alone
@pytest.mark.gpu
@pytest.mark.parametrize("case,call", [(case, call) for case in sorted(CASES) for call in CALLS if call == "gradient" or "d_mu" not in CASES[case][0]])
def test_refusals_keep_their_code_text_and_order(setting, case, call):
    capi, kinds = setting
    faults, winner = CASES[case]
    for kind, (pr, alpha, fresh, ctx) in kinds.items():
        if "error_model" in faults and kind != "plain":
            continue                                         # only a context created without an error model refuses one
        rc, text, _ = _call(capi, ctx, call, pr, faults, alpha=alpha)
        assert (rc, text) == EXPECTED[(call, winner)], (kind, case, call)
        rc, text, got = _call(capi, ctx, call, pr, alpha=alpha)
        assert rc == 0, (kind, case, call, text)
        assert sorted(got) == sorted(fresh[call])
        for key, val in fresh[call].items():
            assert got[key].tobytes() == val.tobytes(), (kind, case, call, key)
