"""The numpy statement of the sum rule and of the root posterior (tests/root_rule_ref.py) against marginal_ref, and what the
inputs of the GPU tests (test_root_rule_gpu.py, test_root_posterior_gpu.py) can tell apart.  No GPU.

Inputs: the six-taxon problem of tests/bd_lm_ref.py at orders 41 and 300, its eight families with three of them repeated (so
that multiplicities matter), a prior ~ 1 / s (so that reading it one place off changes every weight) -- base model, gamma
K = 3 and a 3-tap error model, with lambda = mu and with death rates.  The GPU tolerance is the project's bound for sums
without cancellation, 1e-12 + 1e-10 |ref|; every wrong variant of root_rule_ref.VARIANTS must miss it by a factor of 1000."""
import dataclasses
import functools

import numpy as np
import pytest

import bd_lm_ref as BL
import marginal_ref as MR
import root_rule_ref as RR
from cafexp_amd import problem as P

MODELS = ("base", "gamma", "error")
RATES = {"lambda_eq_mu": None, "death_rates": BL.MUS}
ORDERS = (41, 300)
REPS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 2, 2, 5])            # families 2 and 5 occur three and two times
DISTINCT = np.arange(8)
TIE = 1e-9
MAX_EXCUSED = 0.05                                           # test_gradient_gpu.py's cap


def prior_one_over_s(R):
    w = 1.0 / np.arange(1, R + 1)
    return (w / w.sum()).astype(np.float32)


def repeated(pb, reps):
    return dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[reps]), family_ids=["d%d" % i for i in range(len(reps))])


def case(order, model):
    pb = repeated(BL.problem(order, n_dev=3 if model == "error" else 0), REPS)
    pr = BL.params(pb, model)
    pr.prior = prior_one_over_s(pb.max_root_family_size)
    return pb, pr


def mults(pr):
    return [1.0] if pr.multipliers is None else list(pr.multipliers)


@functools.lru_cache(maxsize=None)
def reference_vectors(order, model, rates):
    """L[f][k][j] of the case from the numpy matrices of bd_lm_ref (the distinct families computed once)"""
    pb, pr = case(order, model)
    mus = BL.LAMBDAS if RATES[rates] is None else RATES[rates]
    mats = BL.reference_matrices(pb, pr.lambdas, mus, mults(pr))
    return RR.root_vectors(pb, pr, mats, families=list(DISTINCT))[REPS]


def differs(a, b, factor=1000.0):
    """True when a misses b by more than factor x the GPU bound somewhere (a NaN where b has a number counts)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.any(~(np.abs(a - b) <= factor * RR.bound(b)) & ~np.isnan(b)))


# the underflow case of test_root_rule_gpu.py: order 300, a Poisson prior far below the counts
UNDERFLOW_ROW = [220, 230, 225, 220, 230, 225]
UNDERFLOW_POISSON = 20.0
UNDERFLOW_LAMBDAS = np.array([0.003, 0.002])


def underflow_case():
    base = BL.problem(300)
    counts = np.array([UNDERFLOW_ROW, list(base.counts[0])], dtype=np.int32)
    pb = dataclasses.replace(base, counts=counts, family_ids=["under", "plain"])
    pr = P.Params(lambdas=UNDERFLOW_LAMBDAS.copy(), prior=P.prior_poisson(pb.max_root_family_size, UNDERFLOW_POISSON))
    return pb, pr


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("rates", sorted(RATES))
@pytest.mark.parametrize("model", MODELS)
def test_the_sum_rule_is_the_log_evidence_of_the_up_down_pass(order, model, rates):
    pb, pr = case(order, model)
    mus = BL.LAMBDAS if RATES[rates] is None else RATES[rates]
    mats = BL.reference_matrices(pb, pr.lambdas, mus, mults(pr))
    L = reference_vectors(order, model, rates)
    got = RR.sum_rule(pr, L)["family_lnl"]
    post = RR.root_posterior(pr, L)
    fams = [0, 3, 7] if order == 300 else list(DISTINCT)     # (the down pass at order 300 is what takes the time)
    want = MR.updown(pb, pr, mats, 0.95, families=fams)
    root = MR.root_of(pb)
    assert not want["failed"].any() and not post["failed"].any()
    assert np.all(np.abs(got[fams] - want["log_evidence"]) <= 1e-12 * np.abs(want["log_evidence"]))
    assert np.all(np.abs(post["log_evidence"][fams] - want["log_evidence"]) <= 1e-12 * np.abs(want["log_evidence"]))
    assert np.all(np.abs(post["mean"][fams] - want["mean"][:, root]) <= 1e-12 * want["mean"][:, root])
    assert np.array_equal(post["mode"][fams], want["mode"][:, root])
    assert np.all(np.abs(post["total"].sum() - post["n_used"]) <= 1e-12 * post["n_used"]) and post["n_used"] == len(REPS)
    assert np.all(np.abs(post["category_posterior"].sum(axis=1) - 1.0) <= 1e-14)
    assert np.array_equal(got[8:], got[REPS[8:]])


@pytest.mark.parametrize("model", MODELS)
def test_an_em_step_never_lowers_the_likelihood(model):
    pb, pr = case(41, model)
    L = reference_vectors(41, model, "death_rates")
    prior = np.asarray(pr.prior, dtype=np.float64)
    before = RR.log_likelihood(pr, L, prior)
    for _ in range(5):
        prior = RR.em_step(pr, L, prior=prior)
        assert abs(prior.sum() - 1.0) <= 1e-13
        after = RR.log_likelihood(pr, L, prior)
        assert after >= before - 1e-12 * abs(before), (before, after)
        before = after
    assert RR.log_likelihood(pr, L, prior) > RR.log_likelihood(pr, L, np.asarray(pr.prior, dtype=np.float64)) + 1.0


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("rates", sorted(RATES))
@pytest.mark.parametrize("model", MODELS)
def test_the_inputs_tell_every_wrong_variant_from_the_right_one(order, model, rates):
    pb, pr = case(order, model)
    L = reference_vectors(order, model, rates).copy()
    L[1] = 0.0                                               # one family made to fail, as a saturated branch does on the device
    right_s, right_p = RR.sum_rule(pr, L), RR.root_posterior(pr, L)
    assert right_p["failed"].sum() == 1 and right_p["n_used"] == len(REPS) - 1
    ok = right_p["failed"] == 0
    for name in RR.VARIANTS:
        wrong_s, wrong_p = RR.sum_rule(pr, L, variant=name), RR.root_posterior(pr, L, variant=name, distinct=DISTINCT)
        if name in ("prior_shifted", "max_for_one_category", "cat_probs_forgotten"):
            if model != "gamma" and name != "prior_shifted":
                continue                                     # (no categories to get wrong)
            assert differs(wrong_s["family_lnl"][ok], right_s["family_lnl"][ok]), name
            if name != "cat_probs_forgotten":                # (the discrete gamma's categories are equally likely: forgetting
                assert differs(wrong_p["total"], right_p["total"]), name        # them is a common factor, the posterior stays)
                assert differs(wrong_p["mean"][ok], right_p["mean"][ok]), name
            if model == "gamma" and name != "prior_shifted":
                assert differs(wrong_s["category_likelihood"][ok], right_s["category_likelihood"][ok]), name
            if model == "gamma" and name == "max_for_one_category":
                assert differs(wrong_p["category_posterior"][ok], right_p["category_posterior"][ok]), name
        else:
            assert differs(wrong_p["total"], right_p["total"]) or wrong_p["n_used"] != right_p["n_used"], name
            assert differs(wrong_p["total"] / wrong_p["n_used"], right_p["total"] / right_p["n_used"]), name


@pytest.mark.parametrize("order", ORDERS)
def test_the_modes_are_not_ties(order):
    gaps = np.concatenate([RR.root_posterior(case(order, m)[1], reference_vectors(order, m, r))["mode_gap"] for m in MODELS for r in RATES])
    share = float((gaps <= TIE).mean())
    print("order %d: smallest relative gap of the two best masses %.3g, share within %.0e: %.3f" % (order, gaps.min(), TIE, share))
    assert share <= MAX_EXCUSED


def test_the_underflow_case_underflows_and_its_log_sum_exp_does_not():
    pb, pr = underflow_case()
    mats = BL.reference_matrices(pb, pr.lambdas, pr.lambdas, [1.0])
    L = RR.root_vectors(pb, pr, mats)
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)
    assert np.all(L[0, 0] * prior == 0.0)                    # every product underflows ...
    with np.errstate(divide="ignore"):
        t = np.log(L[0, 0]) + np.log(prior)
    assert np.isfinite(t).sum() >= 3                         # ... while some of the logarithms are finite
    value = RR.sum_rule(pr, L)["family_lnl"]
    print("underflow case: log-sum-exp %.6f over %d finite terms; the plain family %.6f" % (value[0], int(np.isfinite(t).sum()), value[1]))
    assert np.isfinite(value).all() and value[0] < -745.0    # below log of the smallest double
    post = RR.root_posterior(pr, L)
    assert list(post["failed"]) == [1, 0]


def test_the_new_entries_are_exported_and_the_abi_version_stays():
    from cafexp_amd import capi
    lib = capi.load()
    for name in ("cafe_set_root_rule", "cafe_get_root_rule", "cafe_root_posterior"):
        assert name in capi.EXPORTS and getattr(lib, name) is not None
    assert lib.cafe_abi_version() == 3
    assert lib.cafe_get_root_rule(None) == capi.CAFE_ROOT_MAX and lib.cafe_set_root_rule(None, capi.CAFE_ROOT_SUM) != 0
