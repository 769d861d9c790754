"""The per-family score d log Z_f / d theta (cafe_score_gradient) on the CPU: the two numpy statements of
tests/gradient_ref.py against each other and against central differences, cafe_bd_rates_grad (host code, through ctypes)
against 50-digit arithmetic, the exported symbols, and the command lines the driver refuses.

Inputs: the six-taxon problem of tests/bd_lm_ref.py (a cherry, a trifurcation, a leaf under the root; M = 40, R = 30, two
lambda classes), base model, gamma K = 3 and a 3-tap error model, with lambda = mu, with unequal death rates and with
mus == lambdas, under both root rules.

Bounds.  complex_step against reverse: 1e-12 + 1e-10 c |ref| with c = 1000, the largest cancellation factor reverse
reports on these inputs (742, gamma model with death rates under MAX) rounded up to a power of ten -- the bound of the GPU
tests; the two agree to 1e-13 relative.  Central differences with h = 1e-4 lambda on quantized points, divided by the
actual difference of the quantized rates: 1e-6 relative (truncation is of order (h / lambda)^2 = 1e-8 times a ratio of
derivatives; measured 5e-9) plus the rounding of the quotient itself, 4 eps |lnL| / |difference|."""
import os
import subprocess

import numpy as np
import pytest

import bd_lm_ref as BL
import gradient_ref as GR

C_MODEL = 1000.0
HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
RATES = {"lambda_eq_mu": None, "death_rates": BL.MUS, "mus_eq_lambdas": BL.LAMBDAS}


def _case(model):
    pb = BL.problem(41, n_dev=3 if model == "error" else 0)
    return pb, BL.params(pb, model)


@pytest.mark.parametrize("rule", ["max", "sum"])
@pytest.mark.parametrize("rates", sorted(RATES))
@pytest.mark.parametrize("model", ["base", "gamma", "error"])
def test_the_two_statements_agree(model, rates, rule):
    pb, pr = _case(model)
    cs = GR.complex_step(pb, pr, RATES[rates], rule)
    rv = GR.reverse(pb, pr, RATES[rates], rule)
    assert not cs["failed"].any()
    c = GR.worst_cancellation(rv)
    print("%s %s %s: cancellation factor %.1f" % (model, rates, rule, c))
    assert c <= C_MODEL
    GR.close(rv, cs, C_MODEL, "reverse against complex step")
    GR.close({k.replace("dense_", ""): v for k, v in rv.items() if k.startswith("dense_") or k == "failed"}, cs, C_MODEL, "dense dP against complex step")
    assert np.allclose(rv["family_lnl"], cs["family_lnl"], rtol=1e-13, atol=0)
    for a, b in zip(rv["args"], cs["args"]):
        assert (a is None and b is None) or np.array_equal(a, b)


def test_at_equal_rates_the_partials_add_up_to_the_derivative_along_the_diagonal():
    for model in ("base", "gamma"):
        pb, pr = _case(model)
        for rule in ("max", "sum"):
            both = GR.complex_step(pb, pr, BL.LAMBDAS, rule)
            one = GR.complex_step(pb, pr, None, rule)
            assert np.allclose(both["d_lambda"] + both["d_mu"], one["d_lambda"], rtol=1e-10, atol=1e-12)
            if model == "gamma":
                assert np.allclose(both["d_multiplier"], one["d_multiplier"], rtol=1e-10, atol=1e-12)


def _central(pb, pr, mus, rule, kind, q):
    """(difference quotient per family, arg max unchanged per family, rounding floor per family) of log Z in lambda_q or mu_q"""
    lam0 = np.array(pr.lambdas, dtype=float)
    mu0 = None if mus is None else np.array(mus, dtype=float)
    h = 1e-4 * lam0[q]
    vals, args, pts = [], [], []
    for sign in (-1.0, 1.0):
        lam, mu = lam0.copy(), None if mu0 is None else mu0.copy()
        if kind == "lambda":
            lam[q] += sign * h
            pts.append(BL.quantize(lam[q], 0.0, 0.0)[0])
        else:
            mu[q] += sign * h
            pts.append(BL.quantize(mu[q], 0.0, 0.0)[0])
        p2 = type(pr)(lambdas=lam, prior=pr.prior, multipliers=pr.multipliers, cat_probs=pr.cat_probs, error_model=pr.error_model)
        a = []
        vals.append(GR.log_z(pb, p2, mu, rule, args=a).real)
        args.append(a)
    same = np.ones(pb.n_families, dtype=bool)
    if rule == "max":
        for a, b in zip(*args):
            same &= a == b
    width = pts[1] - pts[0]
    return (vals[1] - vals[0]) / width, same, 4 * np.finfo(float).eps * np.abs(vals[0]) / width


@pytest.mark.parametrize("rule", ["max", "sum"])
@pytest.mark.parametrize("rates", ["lambda_eq_mu", "death_rates"])
@pytest.mark.parametrize("model", ["base", "error"])
def test_each_agrees_with_central_differences_on_quantized_points(model, rates, rule):
    pb, pr = _case(model)
    mus = RATES[rates]
    cs, rv = GR.complex_step(pb, pr, mus, rule), GR.reverse(pb, pr, mus, rule)
    for kind in ["lambda"] + ([] if mus is None else ["mu"]):
        for q in range(pb.n_lambdas):
            fd, same, floor = _central(pb, pr, mus, rule, kind, q)
            assert (~same).sum() <= 0.05 * pb.n_families           # the reference alone stays within the cap
            for name, ref in (("complex step", cs), ("reverse", rv)):
                g = ref["d_" + kind][:, q]
                err = np.abs(fd - g)[same]
                bound = (1e-6 * np.abs(g) + floor)[same]
                print("%s %s %s d_%s[%d] %s: worst |fd - g| / bound %.3g" % (model, rates, rule, kind, q, name, (err / bound).max()))
                assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------- cafe_bd_rates_grad (host code)
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _mp_partials(lam, mu, t):
    """the four partials of alpha = mu (E - 1) / (lambda E - mu), beta = lambda (E - 1) / (lambda E - mu) at the quantized key,
    50 digits: differentiated by mpmath away from equal rates, the limits at equal rates"""
    import mpmath as mp
    lq, mq, tq = BL.quantize(lam, mu, t)
    with mp.workdps(80):
        L, M, T = mp.mpf(lq), mp.mpf(mq), mp.mpf(tq)
        if lq == mq:
            a = -L * T * T / (2 * (1 + L * T) ** 2)
            b = T * (1 + L * T / 2) / (1 + L * T) ** 2
            out = (a, b, b, a)
        else:
            def alpha(l, m):
                return m * mp.expm1((l - m) * T) / (l * mp.exp((l - m) * T) - m)

            def beta(l, m):
                return l * mp.expm1((l - m) * T) / (l * mp.exp((l - m) * T) - m)
            h = mp.mpf(10) ** -30 * max(mp.mpf(1e-3), abs(L - M))     # steps far below the scale the functions vary on, far above 80 digits of noise
            out = (mp.diff(lambda l: alpha(l, M), L, h=h), mp.diff(lambda m: alpha(L, m), M, h=h),
                   mp.diff(lambda l: beta(l, M), L, h=h), mp.diff(lambda m: beta(L, m), M, h=h))
        return [float(mp.nstr(x, 50)) for x in out], tq, lq


GRAD_KEYS = dict(BL.RATES)
GRAD_KEYS.update({"near_1e-3": (0.011, 0.01, 1.0), "near_1e-6": (0.010001, 0.01, 1.0), "near_1e-9": (0.010000001, 0.01, 1.0), "near_1e-12": (0.010000001, 0.01, 0.001), "near_below": (0.01, 0.010000001, 0.5),
                  "equal": (0.0018, 0.0018, 68.7105), "equal_long": (0.01, 0.01, 96.435), "large_x": (0.9, 0.001, 900.0), "large_negative_x": (0.001, 0.9, 900.0)})


@pytest.mark.parametrize("name", sorted(GRAD_KEYS))
def test_bd_rates_grad_matches_50_digit_arithmetic(capi, name):
    """Each partial is a sum of at most three terms of like magnitude built from correctly rounded exp / expm1 and a series
    of positive terms: a few hundred ulps at the worst.  1e-12 relative (plus 1e-300 for the partials that are exactly 0)."""
    lam, mu, t = GRAD_KEYS[name]
    want, tq, lq = _mp_partials(lam, mu, t)
    got = capi.bd_rates_grad(lam, mu, t)
    print(name, got, want)
    assert all(np.isfinite(got))
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w) + 1e-300, (name, got, want)
    if BL.quantize(lam, mu, t)[0] == BL.quantize(lam, mu, t)[1]:
        slope = tq / (1 + lq * tq) ** 2
        assert got[0] + got[1] == pytest.approx(slope, rel=1e-14) and got[2] + got[3] == pytest.approx(slope, rel=1e-14)


def test_the_keys_cover_what_they_should():
    x = {k: abs(BL.quantize(*v)[0] - BL.quantize(*v)[1]) * BL.quantize(*v)[2] for k, v in GRAD_KEYS.items()}
    assert min(v for v in x.values() if v > 0) <= 1.0000001e-12 and max(x.values()) > 700
    assert {"rho_0.25", "rho_0.8", "rho_1.25", "rho_4", "pure_birth", "pure_death"} <= set(GRAD_KEYS)
    assert sum(1 for v in x.values() if v == 0) >= 2


def test_bd_rates_grad_is_continuous_at_equal_rates(capi):
    lam, t = 0.01, 30.0
    at = capi.bd_rates_grad(lam, lam, t)
    for d in (1e-9, 2e-9, 1e-8):
        for pair in ((lam + d, lam), (lam, lam + d)):
            near = capi.bd_rates_grad(pair[0], pair[1], t)
            for a, b in zip(near, at):
                assert abs(a - b) <= 1e-5 * max(abs(at[1]), abs(at[0]))     # the partials vary on the scale of lambda: d / lambda = 1e-6


def test_the_library_exports_both_symbols(capi):
    lib = capi.load()
    assert "cafe_score_gradient" in capi.EXPORTS and "cafe_bd_rates_grad" in capi.EXPORTS
    assert lib.cafe_score_gradient is not None and lib.cafe_bd_rates_grad is not None
    assert lib.cafe_abi_version() == 3
    assert hasattr(capi.Context, "score_gradient") and capi.CAFE_ROOT_MAX == 0 and capi.CAFE_ROOT_SUM == 1


def test_the_driver_refuses_what_does_not_combine(tmp_path):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    data = os.path.join(HERE, "golden", "data")
    common = ["-t", os.path.join(data, "synth20_tree.txt"), "-i", os.path.join(data, "synth20_families.txt"), "-o", str(tmp_path / "out")]
    for extra, message in ((["--standard-errors", "-b"], "-b is not supported with it"),
                           (["--standard-errors", "--gpus", "2"], "--gpus is not supported with it"),
                           (["--standard-errors", "--simulate", "10", "-l", "0.01"], "--simulate is not supported with it")):
        r = subprocess.run([DRIVER] + common + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--standard-errors" in r.stderr and message in r.stderr, (extra, r.stderr)
    assert not os.path.exists(str(tmp_path / "out"))
