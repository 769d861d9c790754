"""Plain numpy statements of the expected number of births and deaths on every branch given the leaf counts (a helper,
not a test): what cafe_expected_events computes.

Tag every birth with a factor r and every death with a factor w.  The single-lineage generating function of the linear
birth-death process stays linear-fractional, phi(z) = a + c z / (1 - b z), with s = lambda + mu, A = lambda r, C = mu w,
D = s^2 - 4 A C, omega = sqrt(D), sh = sinh(omega t / 2) / omega, ch = cosh(omega t / 2), T = s sh + ch:
    a = 2 C sh / T        b = 2 A sh / T        c = (ch - s sh) / T + a b,
and E[births; X_t = j | X_0 = i] = d P_ij / d r at r = w = 1 (deaths: d / d w).  The event matrices of a key, three ways:
  rows      row i of P(r, w) is the i-fold convolution of (a, c, c b, c b^2, ...); r (or w) gets the imaginary part 1e-30 and
            the derivative is Im P / 1e-30: no subtraction, no step-size error.  sh and ch are even in omega, so both are
            evaluated as series in D where |omega t| is small: the step stays analytic at lambda = mu;
  expm      scipy.linalg.expm of the tagged generator Q[i][i+1] = lambda i r, Q[i][i-1] = mu i w, Q[i][i] = -(lambda + mu) i,
            cut far above the sizes read, with the same complex step;
  filters   the statement csrc/events.hip implements: with x = P[i-1], H the causal filter y[j] = x[j] + b y[j-1] and S the
            shift by one,  E[i] = i (da x + dc H S x + db c H H S S x),  (da, db, dc) by a complex step on the three scalars.
            `mutant` makes it deliberately WRONG (MUTANTS).
`reference` contracts them with G, P and B of the up and down passes of gradient_ref / marginal_ref:
    events[v] = sum_k p_k sum_{i, j} G_v[i] E_v[i][j] B_v[j] / Z.
Rates are quantized like the library's keys; mus=None is the lambda = mu model (births and deaths are still told apart).
"""
import numpy as np

import gradient_ref as GR
import marginal_ref as MR

STEP = 1e-30
MUTANTS = ("gains_losses_swapped", "dc_dropped", "c_tied", "b_shift_by_one")


def _sh_ch(D, t):
    """sinh(omega t / 2) / omega and cosh(omega t / 2), omega^2 = D (complex D allowed)"""
    u = D * t * t / 4                                        # (omega t / 2)^2
    if abs(u) < 0.25:
        sh = ch = 0.0
        ts, tc = t / 2, 1.0                                  # u^k / (2k+1)! t/2 and u^k / (2k)!
        for k in range(16):
            sh, ch = sh + ts, ch + tc
            ts = ts * u / ((2 * k + 2) * (2 * k + 3))
            tc = tc * u / ((2 * k + 1) * (2 * k + 2))
        return sh, ch
    om = np.sqrt(complex(D))
    return np.sinh(om * t / 2) / om, np.cosh(om * t / 2)


def coefficients(lam, mu, t, r=1.0, w=1.0, tied=False):
    """(a, b, c) of the tagged process; tied: c = (1 - a)(1 - b), true only at r = w = 1"""
    s, A, C = lam + mu, lam * r, mu * w
    sh, ch = _sh_ch(s * s - 4 * A * C, t)
    T = s * sh + ch
    a, b = 2 * C * sh / T, 2 * A * sh / T
    return a, b, (1 - a) * (1 - b) if tied else (ch - s * sh) / T + a * b


def rows_matrix(n, a, b, c, zero=False):
    one = np.empty(n, dtype=complex)
    one[0] = a
    one[1:] = c * b ** np.arange(n - 1)
    P = np.zeros((n, n), dtype=complex)
    P[0, 0] = 1.0
    if zero:
        return P
    for i in range(1, n):
        P[i] = np.convolve(P[i - 1], one)[:n]
    return P


def _zero(lam, mu, t):
    a, b = GR.alpha_beta(lam, mu, t)
    return GR.is_zero(a, b)


def by_rows(n, lam, mu, t):
    """(P, gains, losses), each [n][n]; a key marked zero has no events"""
    zero = _zero(lam, mu, t)
    P = rows_matrix(n, *coefficients(lam, mu, t), zero=zero).real
    if zero:
        return P, np.zeros((n, n)), np.zeros((n, n))
    g = rows_matrix(n, *coefficients(lam, mu, t, r=1 + 1j * STEP)).imag / STEP
    l = rows_matrix(n, *coefficients(lam, mu, t, w=1 + 1j * STEP)).imag / STEP
    return P, g, l


def by_expm(n, lam, mu, t, big):
    """(P, gains, losses), each [n][n], from the generator cut at `big` sizes"""
    from scipy.linalg import expm
    i = np.arange(big, dtype=float)

    def gen(r, w):
        Q = np.zeros((big, big), dtype=complex)
        Q[np.arange(big - 1), np.arange(1, big)] = lam * i[:-1] * r
        Q[np.arange(1, big), np.arange(big - 1)] = mu * i[1:] * w
        Q[np.arange(big), np.arange(big)] = -(lam + mu) * i
        return Q * t
    return (expm(gen(1.0, 1.0)).real[:n, :n], expm(gen(1 + 1j * STEP, 1.0)).imag[:n, :n] / STEP,
            expm(gen(1.0, 1 + 1j * STEP)).imag[:n, :n] / STEP)


def scalar_derivatives(lam, mu, t, tied=False):
    """((da, db, dc) of the births tag, (da, db, dc) of the deaths tag) at r = w = 1"""
    g = coefficients(lam, mu, t, r=1 + 1j * STEP, tied=tied)
    l = coefficients(lam, mu, t, w=1 + 1j * STEP, tied=tied)
    return tuple(x.imag / STEP for x in g), tuple(x.imag / STEP for x in l)


def by_filters(n, lam, mu, t, mutant=None, parts=False):
    """(P, gains, losses) from the row identities; parts: also the sums of the |terms| of gains and losses"""
    assert mutant is None or mutant in MUTANTS, mutant
    zero = _zero(lam, mu, t)
    a, b, c = (x.real for x in coefficients(lam, mu, t))
    P = rows_matrix(n, a, b, c, zero=zero).real
    if zero:
        z = np.zeros((n, n))
        return (P, z, z, z, z) if parts else (P, z, z)
    dg, dl = scalar_derivatives(lam, mu, t, tied=mutant == "c_tied")
    if mutant == "gains_losses_swapped":
        dg, dl = dl, dg
    prev = np.zeros((n, n))
    prev[1:] = P[:-1]
    x = prev.T                                               # filters run down axis 0
    y1 = GR._H(GR._S(x), b)
    y2 = GR._H(GR._S(y1), b) if mutant != "b_shift_by_one" else GR._H(y1, b)
    i = np.arange(n)[:, None]
    out, absolute = [], []
    for da, db, dc in (dg, dl):
        if mutant == "dc_dropped":
            dc = 0.0
        terms = (da * x.T, dc * y1.T, db * c * y2.T)
        out.append(i * sum(terms))
        absolute.append(i * sum(np.abs(v) for v in terms))
    return (P, out[0], out[1], absolute[0], absolute[1]) if parts else (P, out[0], out[1])


def reference(pb, pr, mus=None, route="filters", mutant=None, big=None):
    """dict: gains, losses [F][n_nodes] (NaN at the root and for a failed family), log_evidence, failed [F], and for the
    filters route cancel_gains / cancel_losses [F][n_nodes]: sum |terms| / |sum terms|, terms = p_k G[i] (one of the three
    parts of E[i][j]) B[j] over categories, i and j (1 where the sum is 0)."""
    n, M, R, N, F = pb.n_nodes, pb.max_family_size, pb.max_root_family_size, pb.matrix_size, pb.n_families
    ch, root = MR.children_of(pb), MR.root_of(pb)
    leafv = GR.leaf_vectors(pb, pr)
    mults, probs = GR._mults(pr), GR._probs(pr)
    acc = np.zeros((2, n, F))
    absacc = np.zeros((2, n, F))
    Z = np.zeros(F)
    for k in range(len(mults)):
        keys, cache, mats = GR.branch_keys(pb, pr, mus, k), {}, [None] * n
        for v in range(n):
            if keys[v] is None:
                continue
            if keys[v] not in cache:
                if route == "filters":
                    cache[keys[v]] = by_filters(N, *keys[v], mutant=mutant, parts=True)
                elif route == "rows":
                    cache[keys[v]] = by_rows(N, *keys[v])
                else:
                    cache[keys[v]] = by_expm(N, *keys[v], big=big or 6 * N)
            mats[v] = cache[keys[v]]
        P = [None if m is None else m[0] for m in mats]
        B, Fp = GR._up(pb, P, leafv, float)
        O = [None] * n
        O[root], _ = GR._root_weight(pb, pr, B[root], "sum", False)
        Z += probs[k] * (O[root] * B[root]).sum(axis=0)
        for p in range(n - 1, -1, -1):
            if pb.leaf_taxon[p] >= 0:
                continue
            top = R if p == root else M
            for v in ch[p]:
                G = O[p].copy()
                for w in ch[p]:
                    if w != v:
                        G = G * Fp[w]
                if pb.leaf_taxon[v] < 0:
                    O[v] = P[v][:top + 1, :M + 1].T @ G
                for q in range(2):
                    acc[q, v] += probs[k] * (G * (mats[v][1 + q][:top + 1, :M + 1] @ B[v])).sum(axis=0)
                    if route == "filters":
                        absacc[q, v] += probs[k] * (G * (mats[v][3 + q][:top + 1, :M + 1] @ B[v])).sum(axis=0)
    bad = ~((Z > 0) & np.isfinite(Z))
    out = {"failed": bad.astype(np.int32)}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["log_evidence"] = np.where(bad, np.nan, np.log(Z))
        for q, name in enumerate(("gains", "losses")):
            val = np.where(bad[None, :], np.nan, acc[q] / Z[None, :])
            val[root] = np.nan
            out[name] = val.T.copy()
            if route == "filters":
                out["cancel_" + name] = np.where(acc[q] != 0, absacc[q] / np.abs(acc[q]), 1.0).T.copy()
    return out


def worst_cancellation(ref):
    ok = ref["failed"] == 0
    return max(float(np.max(ref[k][ok])) for k in ref if k.startswith("cancel_"))


KEYS = ("gains", "losses")


def close(got, ref, c, label=""):
    """The gradient's rule: |got - ref| <= 1e-12 + 1e-10 c |ref| on gains and losses, every entry held to its own
    cancellation factor where `ref` reports it (at most c); the same NaN pattern; failed equal; log_evidence at
    1e-12 + 1e-10 |ref|."""
    assert np.array_equal(np.asarray(got["failed"]), np.asarray(ref["failed"])), label
    worst = 0.0
    for key in KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape, (label, key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key)
        ok = ~np.isnan(r)
        if ok.any():
            factor = np.full(r.shape, float(c))
            if "cancel_" + key in ref:
                factor = np.minimum(factor, np.maximum(1.0, ref["cancel_" + key]))
            worst = max(worst, float((np.abs(g[ok] - r[ok]) / (1e-12 + 1e-10 * factor[ok] * np.abs(r[ok]))).max()))
    print("%s: worst |got - ref| / bound (c = %g) = %.3g" % (label, c, worst))
    assert worst <= 1.0, (label, worst)
    if "log_evidence" in got:
        ok = ref["failed"] == 0
        g, r = np.asarray(got["log_evidence"]), np.asarray(ref["log_evidence"])
        assert np.all(np.isnan(g[~ok])) and np.all(np.abs(g[ok] - r[ok]) <= 1e-12 + 1e-10 * np.abs(r[ok])), label
    return worst
