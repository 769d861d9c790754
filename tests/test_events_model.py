"""Expected gains and losses per branch (cafe_expected_events) on the CPU: the numpy statements of tests/events_ref.py against
each other, cafe_bd_rates_events (host code, through ctypes) against many-digit arithmetic, the identities every entry obeys,
the exported symbols, and what the reference can tell apart.

Inputs: the six-taxon problem of tests/bd_lm_ref.py (M = 40, R = 30, two lambda classes), base model, gamma K = 3 and a 3-tap
error model, with lambda = mu, with unequal death rates and with mus == lambdas.

Bounds.  The three statements against each other: the GPU tests' rule |got - ref| <= 1e-12 + 1e-10 c |ref| with c = 1 -- the
six coefficients (da, db, dc) are non-negative, so the three-term sum and every contraction behind an entry are sums of
non-negative terms (test_the_reference_has_no_cancellation asserts that the reference reports c = 1).  The generator of the
expm statement is cut at 6 N = 246 sizes: with lambda t <= 0.11 a lineage's tail ratio is below 0.1, so what leaves the cut
from a size <= 40 is far below 1e-100."""
import functools

import numpy as np
import pytest

import bd_lm_ref as BL
import events_ref as ER
import marginal_ref as MR
from test_gradient_model import GRAD_KEYS

RATES = {"lambda_eq_mu": None, "death_rates": BL.MUS, "mus_eq_lambdas": BL.LAMBDAS}
KEYS3 = [(0.012, 0.007, 5.0), (0.01, 0.01, 8.0), (0.006, 0.02, 6.0), (0.01, 0.0, 30.0), (0.0, 0.01, 30.0), (0.010000001, 0.01, 9.0)]


def _case(model):
    pb = BL.problem(41, n_dev=3 if model == "error" else 0)
    return pb, BL.params(pb, model)


@functools.lru_cache(maxsize=None)
def _reference(model, rates, route):
    pb, pr = _case(model)
    return ER.reference(pb, pr, RATES[rates], route=route)


@pytest.mark.parametrize("rates", sorted(RATES))
@pytest.mark.parametrize("model", ["base", "gamma", "error"])
def test_the_statements_agree(model, rates):
    rows, ex, fl = (_reference(model, rates, r) for r in ("rows", "expm", "filters"))
    assert not rows["failed"].any()
    ER.close(ex, rows, 1.0, "expm against complex-step rows")
    ER.close(fl, rows, 1.0, "filters against complex-step rows")
    ER.close(fl, ex, 1.0, "filters against expm")
    root = MR.root_of(_case(model)[0])
    assert np.all(np.isnan(rows["gains"][:, root])) and np.isfinite(np.delete(rows["gains"], root, axis=1)).all()


def test_the_reference_has_no_cancellation():
    for model in ("base", "gamma", "error"):
        for rates in RATES:
            assert ER.worst_cancellation(_reference(model, rates, "filters")) <= 1.0 + 1e-12


def test_equal_death_rates_are_the_unset_model():
    for model in ("base", "gamma"):
        one, both = _reference(model, "lambda_eq_mu", "rows"), _reference(model, "mus_eq_lambdas", "rows")
        for key in ER.KEYS:
            assert np.array_equal(one[key], both[key], equal_nan=True)


@pytest.mark.parametrize("key", KEYS3)
def test_every_entry_obeys_gains_minus_losses_and_is_not_negative(key):
    """births - deaths = X_t - X_0 on every path, so gains - losses = (j - i) P_ij entry by entry; the bound is 1e-14 of the
    entries' scale (each is a sum of at most n terms of one sign, rounded once per term)."""
    n = 41
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    for route in (ER.by_rows, ER.by_filters):
        P, g, l = route(n, *key)
        assert g.min() >= 0.0 and l.min() >= 0.0
        assert np.all(np.abs(g - l - (j - i) * P) <= 1e-14 * (g + l + 1e-300) + 1e-300), route.__name__
        assert g[0].max() == 0.0 and l[0].max() == 0.0                   # nothing is born of nothing
    if key[0] == 0.0:
        assert g.max() == 0.0 and l.max() > 0.0                          # pure death: no births
    if key[1] == 0.0:
        assert l.max() == 0.0 and g.max() > 0.0


def test_expected_events_of_one_lineage_match_the_textbook():
    """lambda = mu: E[births] = E[deaths] = lambda t per starting lineage, summed over all end sizes (cut far out)"""
    lam, t, n = 0.01, 8.0, 200
    P, g, l = ER.by_rows(n, lam, lam, t)
    assert g[1].sum() == pytest.approx(lam * t, rel=1e-12) and l[1].sum() == pytest.approx(lam * t, rel=1e-12)
    assert g[3].sum() == pytest.approx(3 * lam * t, rel=1e-12)


# ------------------------------------------------------------------------------------------- cafe_bd_rates_events (host code)
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _mp_coefficients(lam, mu, t):
    """the six derivatives at the quantized key by mpmath's central differences of (a, b, c)(r, w) written out as in the
    issue.  c = (ch - s sh) / T + a b is a difference of O(1) numbers that equals 1 / T^2 ~ e^(-omega t): at omega t = 810 it
    loses 350 digits, so the arithmetic carries 1000 and the steps are 1e-300 of the scale the functions vary on."""
    import mpmath as mp
    lq, mq, tq = BL.quantize(lam, mu, t)
    with mp.workdps(1000):
        L, M, T = mp.mpf(lq), mp.mpf(mq), mp.mpf(tq)

        def abc(r, w):
            s, A, Cc = L + M, L * r, M * w
            D = s * s - 4 * A * Cc
            if D == 0:
                sh, ch = T / 2, mp.mpf(1)
            else:
                om = mp.sqrt(D)
                sh, ch = mp.sinh(om * T / 2) / om, mp.cosh(om * T / 2)
            tt = s * sh + ch
            a, b = 2 * Cc * sh / tt, 2 * A * sh / tt
            return a, b, (ch - s * sh) / tt + a * b
        h = mp.mpf(10) ** -300
        out = []
        for tag in (lambda x: abc(x, 1), lambda x: abc(1, x)):
            for idx in range(3):
                out.append(mp.re(mp.diff(lambda x: tag(x)[idx], 1, h=h)))
        return [float(mp.nstr(x, 50)) for x in out]


@pytest.mark.parametrize("name", sorted(GRAD_KEYS))
def test_bd_rates_events_matches_many_digit_arithmetic(capi, name):
    """Each coefficient is a sum of at most two non-negative terms built from correctly rounded exp / expm1 and series of positive
    terms: a few hundred ulps at the worst.  1e-12 relative (plus 1e-300 for the ones that are exactly 0 or underflow), the
    bound cafe_bd_rates_grad is held to."""
    lam, mu, t = GRAD_KEYS[name]
    want = _mp_coefficients(lam, mu, t)
    got = capi.bd_rates_events(lam, mu, t)
    print(name, got, want)
    assert all(np.isfinite(got)) and min(got) >= 0.0
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w) + 1e-300, (name, got, want)
    if BL.quantize(lam, mu, t)[0] == BL.quantize(lam, mu, t)[1]:
        assert got[0] == got[4] and got[1] == got[3] and got[2] == got[5]


def test_the_keys_cover_what_they_should():
    x = {k: abs(BL.quantize(*v)[0] - BL.quantize(*v)[1]) * BL.quantize(*v)[2] for k, v in GRAD_KEYS.items()}
    assert min(v for v in x.values() if v > 0) <= 1.0000001e-12 and max(x.values()) >= 800
    assert sum(1 for v in x.values() if v == 0) >= 2
    assert any(0 < v < 2 for v in x.values()) and any(v > 2 for v in x.values())      # either side of both series' thresholds


def test_bd_rates_events_is_continuous_at_equal_rates(capi):
    lam, t = 0.01, 30.0
    at = capi.bd_rates_events(lam, lam, t)
    for d in (1e-9, 2e-9, 1e-8):
        for pair in ((lam + d, lam), (lam, lam + d)):
            near = capi.bd_rates_events(pair[0], pair[1], t)
            for a, b in zip(near, at):
                assert abs(a - b) <= 1e-5 * max(at)                      # they vary on the scale of lambda: d / lambda = 1e-6


def test_bd_rates_events_agrees_with_the_reference_scalars(capi):
    for key in KEYS3:
        g, l = ER.scalar_derivatives(*BL.quantize(*key))
        for got, want in zip(capi.bd_rates_events(*key), g + l):
            assert abs(got - want) <= 1e-12 * abs(want) + 1e-300, key


def test_the_library_exports_both_symbols(capi):
    lib = capi.load()
    assert "cafe_expected_events" in capi.EXPORTS and "cafe_bd_rates_events" in capi.EXPORTS
    assert lib.cafe_expected_events is not None and lib.cafe_bd_rates_events is not None
    assert lib.cafe_abi_version() == 3
    assert hasattr(capi.Context, "expected_events")
    assert [n for n, _ in capi.CafeEventsOut._fields_] == ["gains", "losses", "log_evidence", "failed"]


# ------------------------------------------------------------------------------------------- what the reference can tell apart
@pytest.mark.parametrize("rates", ["lambda_eq_mu", "death_rates"])
@pytest.mark.parametrize("model", ["base", "gamma", "error"])
def test_the_inputs_tell_a_wrong_statement_from_the_right_one(model, rates):
    pb, pr = _case(model)
    ref = _reference(model, rates, "filters")
    for name in ER.MUTANTS:
        mut = ER.reference(pb, pr, RATES[rates], mutant=name)
        ratio = max(np.nanmax(np.abs(mut[k] - ref[k]) / (1e-12 + 1e-10 * np.abs(ref[k]))) for k in ER.KEYS)
        print("%s %s %s: %.3g x the bound" % (name, model, rates, ratio))
        assert ratio > 100, name
        with pytest.raises(AssertionError):
            ER.close(mut, ref, 1.0, name)
