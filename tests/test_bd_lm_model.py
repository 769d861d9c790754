"""Separate birth and death rates, the CPU side: the numpy reference (tests/bd_lm_ref.py) pinned to itself and to the oracle, the
identity the k-major build relies on checked numerically, cafe_bd_rates through ctypes (host code: no GPU), and what the GPU
matrix test's inputs can tell apart."""
import math

import numpy as np
import pytest

import bd_lm_ref as R

RHO = (0.25, 0.8, 1.25, 4.0)


def _ab(rho, mu=0.01, t=25.0):
    a, b, zero = R.rates(rho * mu, mu, t)
    assert not zero
    return a, b


@pytest.mark.parametrize("rho", RHO)
def test_closed_form_and_convolution_agree(rho):
    a, b = _ab(rho)
    for n in (3, 16, 65):
        want = R.closed_form(n, a, b)
        assert R.worst_rel(R.by_convolve(n, a, b), want) <= 1e-12
        assert R.worst_rel(R.by_filter(n, a, b), want) <= 1e-12
    assert np.abs(want[:3].sum(axis=1) - 1).max() <= 1e-9    # order 65: the first rows lose nothing to the truncation


@pytest.mark.parametrize("lam,t", [(0.05, 5.0), (0.006335, 68.7105), (0.02, 25.0)])
def test_closed_form_at_equal_rates_is_the_oracles_matrix(oracle, lam, t):
    a, b, zero = R.rates(lam, lam, t)
    assert a == b and not zero
    for n in (5, 33, 65):
        want = oracle.build_matrix(n, lam, t)
        assert R.worst_rel(R.closed_form(n, a, b), want) <= 1e-11
        assert R.worst_rel(R.matrix(n, lam, lam, t), want) <= 1e-11


@pytest.mark.parametrize("rho", RHO)
def test_swap_identity(rho):
    """P_{lambda,mu}[s][c] c = s P_{mu,lambda}[c][s]: exchanging the rates exchanges alpha and beta"""
    a, b = _ab(rho)
    a2, b2, _ = R.rates(0.01, rho * 0.01, 25.0)
    assert abs(a2 - b) <= 1e-15 and abs(b2 - a) <= 1e-15
    for n in (16, 65):
        P, Q = R.closed_form(n, a, b), R.closed_form(n, b, a)
        s = np.arange(n)[:, None].astype(float)
        c = np.arange(n)[None, :].astype(float)
        lhs, rhs = P * c, s * Q.T
        big = rhs > 1e-290
        assert (np.abs(lhs - rhs)[big] / rhs[big]).max() <= 1e-11
        # ... and the k-major build as the kernel runs it (exchanged recurrence, s/c, the two places that are not exchanged)
        assert R.worst_rel(R.kmajor_emulation(n, a, b), P) <= 1e-12


def test_pure_birth_and_pure_death():
    n = 40
    a, b, zero = R.rates(0.01, 0.0, 30.0)                    # pure birth: negative binomial, nothing below the diagonal
    assert a == 0.0 and not zero and abs(b - (1 - math.exp(-0.3))) <= 1e-15
    P = R.by_convolve(n, a, b)
    assert not np.tril(P, -1).any()
    for s, c in [(1, 1), (3, 7), (5, 5), (2, 30)]:
        assert P[s, c] == pytest.approx(math.comb(c - 1, s - 1) * (1 - b) ** s * b ** (c - s), rel=1e-12)
    assert R.worst_rel(R.closed_form(n, a, b), P) <= 1e-12 and R.worst_rel(R.kmajor_emulation(n, a, b), P) <= 1e-12
    a, b, zero = R.rates(0.0, 0.01, 30.0)                    # pure death (several-lambda validity): binomial thinning
    assert b == 0.0 and not zero and abs(a - (1 - math.exp(-0.3))) <= 1e-15
    P = R.by_convolve(n, a, b)
    assert not np.triu(P, 1).any()
    for s, c in [(1, 0), (1, 1), (7, 3), (30, 30)]:
        assert P[s, c] == pytest.approx(math.comb(s, c) * (1 - a) ** c * a ** (s - c), rel=1e-12)
    assert np.abs(P.sum(axis=1) - 1).max() <= 1e-12
    assert R.worst_rel(R.closed_form(n, a, b), P) <= 1e-12 and R.worst_rel(R.kmajor_emulation(n, a, b), P) <= 1e-12


# ------------------------------------------------------------------ cafe_bd_rates (ctypes, host code)
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def test_bd_rates_at_equal_rates_has_todays_bits(capi):
    for lam, t in [(0.0018, 68.7105), (0.01, 96.435575), (0.5, 1.0), (1e-5, 0.01), (0.0053, 53.667), (0.9, 7.0), (0.0, 3.0)]:
        lq, _, tq = R.quantize(lam, lam, t)
        alpha = lq * tq / (1 + lq * tq)                      # slot_param (cafe_kernels.h), the same IEEE operations
        coeff = 1 - 2 * alpha
        a, b, zero = capi.bd_rates(lam, lam, t)
        assert a == alpha and b == alpha and zero == (not (coeff > 0 and coeff != 1)), (lam, t)
    a, b, zero = capi.bd_rates(0.0100000001, 0.0100000009, 10.0)         # rates that quantize alike are equal rates
    assert a == b == capi.bd_rates(0.01, 0.01, 10.0)[0]


def test_bd_rates_is_finite_and_below_one_over_the_whole_range(capi):
    for x in (1e-12, 1e-9, 1e-6, 1e-3, 0.1, 1.0, 10.0, 37.0, 100.0, 709.0, 800.0):
        for lo in (0.0, 1e-9, 0.003, 0.5):
            for t in (0.001, 1.0, 1000.0):
                d = x / t
                if d < 1e-9:                                  # below the quantum the rates are equal: covered above
                    continue
                for lam, mu in ((lo + d, lo), (lo, lo + d)):
                    a, b, zero = capi.bd_rates(lam, mu, t)
                    assert math.isfinite(a) and math.isfinite(b) and 0.0 <= a < 1.0 and 0.0 <= b < 1.0, (lam, mu, t, a, b)
                    ra, rb, rz = R.rates(lam, mu, t)
                    # expm1 within an ulp, then a product, a sum and a quotient: 8 eps
                    assert abs(a - ra) <= 1e-15 * ra and abs(b - rb) <= 1e-15 * rb, (lam, mu, t, a, ra, b, rb)
                    if abs(1 - ra - rb) > 1e-12 and abs(ra + rb) > 1e-12:     # away from the two edges of the rule the flag is the reference's
                        assert zero == rz, (lam, mu, t)


def test_bd_rates_is_continuous_at_equal_rates(capi):
    lam, t = 0.004, 50.0
    a0 = capi.bd_rates(lam, lam, t)[0]
    last = None
    for k in (1000000, 100000, 10000, 1000, 100, 10, 1):    # |lambda - mu| in quanta of 1e-9
        d = k * 1e-9
        diffs = []
        for lm in ((lam + d, lam), (lam, lam + d), (lam - d, lam), (lam, lam - d)):
            a, b, zero = capi.bd_rates(lm[0], lm[1], t)
            assert not zero
            diffs += [abs(a - a0), abs(b - a0)]
        worst = max(diffs)
        assert worst <= t * (d + 1e-9)                        # a rate enters through rate x t only, with slope <= 1; + one quantum of the key
        assert last is None or worst < last
        last = worst


def test_zero_flag_follows_coeff(capi):
    assert capi.bd_rates(0.0, 0.0, 10.0)[2]                               # lambda = mu = 0: degenerate, as today
    assert capi.bd_rates(0.01, 0.004, 0.0)[2]                             # t_q = 0: coeff = 1
    assert capi.bd_rates(*R.SATURATED)[2] and R.rates(*R.SATURATED)[2]
    for key in R.RATES.values():
        assert not capi.bd_rates(*key)[2] and not R.rates(*key)[2]


# ------------------------------------------------------------------ what the GPU matrix test's inputs can see
WRONG = {
    "row-major with alpha and beta exchanged": lambda n, a, b: R.by_filter(n, b, a),
    "k-major not exchanged": lambda n, a, b: R.kmajor_emulation(n, a, b, exchange=False, left_from="alpha"),
    "stored row 0 from beta": lambda n, a, b: R.kmajor_emulation(n, a, b, row0_from="beta"),
    "left neighbour from alpha": lambda n, a, b: R.kmajor_emulation(n, a, b, left_from="alpha"),
}


@pytest.mark.parametrize("name", sorted(R.RATES))
def test_each_mistake_shows_at_every_gpu_order(name):
    """At the (lambda, mu, t) and orders of the GPU matrix test each wrong build differs from the reference by more than the
    GPU tolerance in that test's own metric.  Built at orders 3, 16, 65 and 129: of a larger order only its leading 129 x 129
    block would be built, which is the order-129 matrix itself, and the metric is a maximum over entries, so what shows in
    the block shows in every larger matrix.  None of the four orders is an exception."""
    a, b, zero = R.rates(*R.RATES[name])
    assert not zero and 1 - a - b > 0
    for m in sorted({min(n, 129) for n in R.ORDERS}):
        n = m
        want = R.by_filter(m, a, b)
        assert not R.differs(R.kmajor_emulation(m, a, b), want, 1e-12)
        for what, build in WRONG.items():
            assert R.differs(build(m, a, b), want, 1e3 * R.VEC_TOL), (name, n, what)


# ------------------------------------------------------------------ the GPU tests' numpy prune, pinned where an oracle exists
@pytest.mark.parametrize("order", [41, 300])
def test_the_numpy_prune_of_the_gpu_tests_is_the_oracles_at_equal_rates(oracle, order):
    """tests/test_bd_lm_gpu.py compares the device with a numpy prune (tests/marginal_ref.py) on the reference matrices.  At
    mu = lambda that prune, the scorer's reduction, the root maxima and the Pupko states written for it must be the CPU oracle's."""
    import marginal_ref as MR
    from cafexp_amd import problem as P
    for model in ("base", "gamma", "error"):
        pb = R.problem(order, n_dev=3 if model == "error" else 0)
        pr = R.params(pb, model)
        mults = [1.0] if pr.multipliers is None else list(pr.multipliers)
        ref = MR.updown(pb, pr, R.reference_matrices(pb, R.LAMBDAS, R.LAMBDAS, mults), 0.95)
        got, want = R.score_from_root_vectors(pr, ref["root_inside"]), oracle.score(pb, pr)
        assert abs(got - want) <= 1e-12 * abs(want), (model, got, want)
    pb = R.problem(order)
    pr = R.params(pb, "base")
    mats = R.reference_matrices(pb, R.LAMBDAS, R.LAMBDAS, [1.0])
    ref = MR.updown(pb, pr, mats, 0.95)
    rm = oracle.root_max(pb, R.LAMBDAS)
    assert np.all(np.abs(np.array([fam[0].max() for fam in ref["root_inside"]]) - rm) <= 1e-11 * rm)
    M, Rr = pb.max_family_size, pb.max_root_family_size
    root_prior = np.concatenate(([0.0], P.prior_uniform(Rr)))[:min(M, Rr) + 1].astype(np.float32)
    want = oracle.reconstruct(pb, R.LAMBDAS, root_prior)[0]
    assert np.array_equal(np.array([R.pupko(pb, mats[0], root_prior, f) for f in range(pb.n_families)]), want)
    # and under the death rates of the GPU tests every family has a finite likelihood
    lm = MR.updown(pb, pr, R.reference_matrices(pb, R.LAMBDAS, R.MUS, [1.0]), 0.95)
    assert not lm["failed"].any() and np.isfinite(R.score_from_root_vectors(pr, lm["root_inside"]))
