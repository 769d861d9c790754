"""Plain numpy statements of the per-family score d log Z_f / d theta (a helper, not a test).

Two routes, neither of them the kernels':
  complex_step   a plain prune in complex arithmetic: the free rate gets the imaginary part 1e-30, alpha and beta follow
                 from the textbook formulas, the matrices are rows convolved with the single-lineage law (bd_lm_ref.p1 /
                 by_convolve, restated for complex numbers), the arg max under the MAX rule is taken on real parts, and
                 the derivative is Im(log Z) / 1e-30: no subtraction, no step-size error;
  reverse        the statement csrc/gradient.hip implements: up and down passes, Bt = (da/dtheta) D^T H^T B -
                 (db/dtheta)(1 - alpha) D^T S^T H^T H^T B by two anti-causal scans, Ft = P Bt, sum_{i >= 1} i G[i] Ft[i-1]
                 per branch.  It also forms dP/dtheta densely from the row identities dP/da[i] = i H D P[i-1],
                 dP/db[i] = -i (1 - alpha) H H S D P[i-1], contracts it both ways (the same number again) and reports
                 each family's cancellation factor sum |terms| / |sum terms|, terms = p_k w G[i] dP[i][j] B[j] over
                 categories, branches, i and j.  `mutant` makes one deliberately WRONG pass (MUTANTS).

Rates are quantized like the library's keys (bd_lm_ref.quantize); the derivative is that of the smooth likelihood at the
quantized point.  mus=None is the lambda = mu model, differentiated along lambda = mu.
"""
import numpy as np

import bd_lm_ref as BL
import marginal_ref as MR

STEP = 1e-30
MUTANTS = ("beta_scan_causal", "shift_dropped", "sum_from_zero", "root_unrestricted")


def _q9(x):
    return int(x * 1000000000) / 1000000000.0


def alpha_beta(lam, mu, t):
    """alpha, beta of the (already quantized) key; complex arguments allowed.  Equal real rates with equal imaginary
    parts: lambda t / (1 + lambda t)."""
    lam, mu = complex(lam), complex(mu)
    if lam == mu:
        a = lam * t / (1 + lam * t)
        return a, a
    e1 = np.expm1((lam - mu) * t)
    d = lam * e1 + (lam - mu)                                # (not lam (e1 + 1) - mu: 1 + e1 drops e1's second-order real part)
    return mu * e1 / d, lam * e1 / d


def is_zero(a, b):
    coeff = 1 - a.real - b.real
    return not (coeff > 0 and coeff != 1)


def matrix(n, a, b, zero):
    """by_convolve for complex alpha, beta: row s = row s-1 convolved with p1, cut at n"""
    one = np.empty(n, dtype=complex)
    one[0] = a
    one[1:] = (1 - a) * (1 - b) * b ** np.arange(n - 1)
    P = np.zeros((n, n), dtype=complex)
    P[0, 0] = 1.0
    if zero:
        return P
    for s in range(1, n):
        P[s] = np.convolve(P[s - 1], one)[:n]
    return P


def _mults(pr):
    return [1.0] if pr.multipliers is None else [float(m) for m in pr.multipliers]


def _probs(pr):
    return [1.0] if pr.cat_probs is None else [float(p) for p in pr.cat_probs]


def branch_keys(pb, pr, mus, k):
    """per node: (lambda_q, mu_q, t_q) of category k, None at the root"""
    m = _mults(pr)[k]
    out = []
    for v in range(pb.n_nodes):
        if pb.parent[v] < 0:
            out.append(None)
            continue
        i = int(pb.lambda_index[v])
        lq = _q9(float(pr.lambdas[i]) * m)
        mq = lq if mus is None else _q9(float(mus[i]) * m)
        out.append((lq, mq, int(float(pb.branch_length[v]) * 1000) / 1000.0))
    return out


def leaf_vectors(pb, pr):
    return {v: np.stack([MR.leaf_vector(pb, pr, f, v) for f in range(pb.n_families)], axis=1)
            for v in range(pb.n_nodes) if pb.leaf_taxon[v] >= 0}


def _up(pb, P, leafv, dtype):
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    ch, root = MR.children_of(pb), MR.root_of(pb)
    B, F = [None] * n, [None] * n
    for v in range(n):
        if pb.leaf_taxon[v] >= 0:
            B[v] = leafv[v].astype(dtype)
            continue
        top = R if v == root else M
        b = np.ones((top + 1, pb.n_families), dtype=dtype)
        for c in ch[v]:
            F[c] = P[c][:top + 1, :M + 1] @ B[c]
            b = b * F[c]
        B[v] = b
    return B, F


def _root_weight(pb, pr, Broot, rule, use_log, restrict=True):
    """O_root [R+1][F] and the arg max per family (None for the sum rule); comparisons on real parts, first maximum"""
    R = pb.max_root_family_size
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)[:R]
    O = np.zeros((R + 1, Broot.shape[1]))
    if rule == "sum":
        O[1:] = prior[:, None]
        return O, None
    with np.errstate(divide="ignore"):
        val = np.log(Broot[1:].real) + np.log(prior)[:, None] if use_log else Broot[1:].real * prior[:, None]
    arg = 1 + np.argmax(val, axis=0)
    if restrict:
        O[arg, np.arange(Broot.shape[1])] = prior[arg - 1]
    else:
        O[1:] = prior[:, None]
    return O, arg


def _parameters(pb, pr, mus):
    par = [("lambda", q) for q in range(pb.n_lambdas)]
    if mus is not None:
        par += [("mu", q) for q in range(pb.n_lambdas)]
    if pr.multipliers is not None:
        par += [("multiplier", k) for k in range(len(pr.multipliers))]
    return par


def _empty(pb, pr, mus):
    F, nl = pb.n_families, pb.n_lambdas
    out = {"d_lambda": np.zeros((F, nl))}
    if mus is not None:
        out["d_mu"] = np.zeros((F, nl))
    if pr.multipliers is not None:
        out["d_multiplier"] = np.zeros((F, len(pr.multipliers)))
    return out


def log_z(pb, pr, mus, rule, leafv=None, bump=None, args=None):
    """log Z per family, complex when `bump` = (kind, index) puts STEP on the imaginary axis of that parameter.  `args`:
    a list that receives the arg max per category (MAX rule)."""
    n, N = pb.n_nodes, pb.matrix_size
    root = MR.root_of(pb)
    leafv = leaf_vectors(pb, pr) if leafv is None else leafv
    use_log = pr.multipliers is None and rule == "max"
    z = 0.0
    lbest = None
    for k, (m, p) in enumerate(zip(_mults(pr), _probs(pr))):
        keys, cache, P = branch_keys(pb, pr, mus, k), {}, [None] * n
        for v in range(n):
            if keys[v] is None:
                continue
            lq, mq, tq = keys[v]
            dl = dm = 0.0
            i = int(pb.lambda_index[v])
            if bump is not None:
                kind, idx = bump
                if kind == "lambda" and idx == i:
                    dl = m
                    dm = m if mus is None else 0.0
                elif kind == "mu" and idx == i:
                    dm = m
                elif kind == "multiplier" and idx == k:
                    dl = float(pr.lambdas[i])
                    dm = dl if mus is None else float(mus[i])
            key = (lq, mq, tq, dl, dm)
            if key not in cache:
                a0, b0 = alpha_beta(lq, mq, tq)
                a, b = alpha_beta(lq + 1j * STEP * dl, mq + 1j * STEP * dm, tq)
                cache[key] = matrix(N, a, b, is_zero(a0, b0))
            P[v] = cache[key]
        B, _ = _up(pb, P, leafv, complex)
        O, arg = _root_weight(pb, pr, B[root], rule, use_log)
        if args is not None:
            args.append(arg)
        zk = (O * B[root]).sum(axis=0)
        z = z + p * zk
        if use_log:
            lbest = np.log(zk)
    with np.errstate(divide="ignore", invalid="ignore"):
        return lbest if use_log else np.log(z)


def complex_step(pb, pr, mus=None, rule="max"):
    """dict: family_lnl, failed, d_lambda [F][n_lambdas], d_mu (with mus), d_multiplier [F][K] (gamma), args"""
    leafv = leaf_vectors(pb, pr)
    args = []
    base = log_z(pb, pr, mus, rule, leafv, args=args)
    out = _empty(pb, pr, mus)
    out["args"] = args
    out["family_lnl"] = base.real.copy()
    out["failed"] = (~np.isfinite(base.real)).astype(np.int32)
    for kind, idx in _parameters(pb, pr, mus):
        out["d_" + kind][:, idx] = log_z(pb, pr, mus, rule, leafv, bump=(kind, idx)).imag / STEP
    for key in ("family_lnl", "d_lambda", "d_mu", "d_multiplier"):
        if key in out:
            out[key][out["failed"] == 1] = np.nan
    return out


# ------------------------------------------------------------------------------------------------- the reverse-mode statement
def _H(x, beta):
    """causal y[j] = x[j] + beta y[j-1] down axis 0"""
    y = np.zeros_like(x)
    acc = np.zeros_like(x[0])
    for j in range(x.shape[0]):
        acc = x[j] + beta * acc
        y[j] = acc
    return y


def _Ht(x, beta):
    """anti-causal w[j] = x[j] + beta w[j+1]"""
    return _H(x[::-1], beta)[::-1]


def _S(x):
    y = np.zeros_like(x)
    y[1:] = x[:-1]
    return y


def _St(x):
    y = np.zeros_like(x)
    y[:-1] = x[1:]
    return y


def scanned(Bv, alpha, beta, da, db, mutant=None):
    """Bt = da D^T H^T B - db (1 - alpha) D^T S^T H^T H^T B"""
    w1 = _Ht(Bv, beta)
    w2 = _H(w1, beta) if mutant == "beta_scan_causal" else _Ht(w1, beta)
    u = da * w1 - db * (1 - alpha) * (w2 if mutant == "shift_dropped" else _St(w2))
    return u - _St(u)


def dense_derivative(Pv, alpha, beta, da, db):
    """dP/dtheta [i][j] = da i (H D P[i-1])[j] - db (1 - alpha) i (H H S D P[i-1])[j], filters along j"""
    rows, cols = Pv.shape
    prev = np.zeros((rows, cols))
    prev[1:] = Pv[:-1]                                       # row i holds P[i-1]
    x = prev.T                                               # filters run down axis 0
    y = _H(x - _S(x), beta)
    z = _H(_S(y), beta)
    i = np.arange(rows)[:, None]
    return i * (da * y.T - db * (1 - alpha) * z.T)


def reverse(pb, pr, mus=None, rule="max", mutant=None):
    """The same dict as complex_step plus cancel_<name> [F][...]: sum |terms| / |sum terms| per entry (inf where the sum is
    0), and dense_<name>: the same derivative from the dense dP contraction."""
    assert mutant is None or mutant in MUTANTS, mutant
    n, M, R, N, F, nl = pb.n_nodes, pb.max_family_size, pb.max_root_family_size, pb.matrix_size, pb.n_families, pb.n_lambdas
    ch, root = MR.children_of(pb), MR.root_of(pb)
    leafv = leaf_vectors(pb, pr)
    mults, probs = _mults(pr), _probs(pr)
    K = len(mults)
    n_par = 1 if mus is None else 2
    use_log = pr.multipliers is None and rule == "max"
    acc = np.zeros((K, nl, n_par, F))
    dense = np.zeros((K, nl, n_par, F))
    absacc = np.zeros((K, nl, n_par, F))
    Z = np.zeros(F)
    lbest, args = None, []
    for k in range(K):
        keys, P, rates, cache = branch_keys(pb, pr, mus, k), [None] * n, [None] * n, {}
        for v in range(n):
            if keys[v] is None:
                continue
            lq, mq, tq = keys[v]
            if keys[v] not in cache:
                a, b = alpha_beta(lq, mq, tq)
                zero = is_zero(a, b)
                d = []                                       # (da, db) per free rate, by a complex step on the scalars
                for dl, dm in ([(1.0, 1.0)] if mus is None else [(1.0, 0.0), (0.0, 1.0)]):
                    a1, b1 = alpha_beta(lq + 1j * STEP * dl, mq + 1j * STEP * dm, tq)
                    d.append((a1.imag / STEP, b1.imag / STEP))
                cache[keys[v]] = (matrix(N, a, b, zero).real, (a.real, b.real, zero, d))
            P[v], rates[v] = cache[keys[v]]
        B, Fp = _up(pb, P, leafv, float)
        O = [None] * n
        O[root], arg = _root_weight(pb, pr, B[root], rule, use_log, restrict=mutant != "root_unrestricted")
        args.append(arg)
        zk = (O[root] * B[root]).sum(axis=0) if mutant != "root_unrestricted" or rule == "sum" else \
            (_root_weight(pb, pr, B[root], rule, use_log)[0] * B[root]).sum(axis=0)
        Z += probs[k] * zk
        if use_log:
            with np.errstate(divide="ignore"):
                lbest = np.log(zk)
        for p in range(n - 1, -1, -1):
            if pb.leaf_taxon[p] >= 0:
                continue
            top = R if p == root else M
            for v in ch[p]:
                G = O[p].copy()
                for w in ch[p]:
                    if w != v:
                        G = G * Fp[w]
                Pv = P[v][:top + 1, :M + 1]
                if pb.leaf_taxon[v] < 0:
                    O[v] = Pv.T @ G
                a, b, zero, d = rates[v]
                if zero:
                    continue
                q = int(pb.lambda_index[v])
                i = np.arange(top + 1)[:, None]
                for t, (da, db) in enumerate(d):
                    Ft = Pv @ scanned(B[v], a, b, da, db, mutant)
                    if mutant == "sum_from_zero":
                        term = (i * G * Ft).sum(axis=0)
                    else:
                        term = (i[1:] * G[1:] * Ft[:-1]).sum(axis=0)
                    acc[k, q, t] += probs[k] * term
                    dP = dense_derivative(Pv, a, b, da, db)
                    dense[k, q, t] += probs[k] * (G * (dP @ B[v])).sum(axis=0)
                    absacc[k, q, t] += probs[k] * (np.abs(G) * (np.abs(dP) @ np.abs(B[v]))).sum(axis=0)
    bad = ~((Z > 0) & np.isfinite(Z))
    out = _empty(pb, pr, mus)
    out["args"] = args
    out["failed"] = bad.astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["family_lnl"] = np.where(bad, np.nan, lbest if use_log else np.log(Z))
        lam = np.asarray(pr.lambdas, dtype=float)
        mu = lam if mus is None else np.asarray(mus, dtype=float)
        m = np.array(mults)

        def combine(x, absolute=False):
            res = {}
            w = np.abs(m) if absolute else m
            res["d_lambda"] = np.einsum("k,kqf->fq", w, x[:, :, 0])
            if mus is not None:
                res["d_mu"] = np.einsum("k,kqf->fq", w, x[:, :, 1])
            if pr.multipliers is not None:
                dm = np.einsum("q,kqf->fk", lam, x[:, :, 0])
                if mus is not None:
                    dm = dm + np.einsum("q,kqf->fk", mu, x[:, :, 1])
                res["d_multiplier"] = dm
            return res
        val, den, ab = combine(acc), combine(dense), combine(absacc, absolute=True)
        for key in val:
            out[key] = np.where(bad[:, None], np.nan, val[key] / Z[:, None])
            out["dense_" + key] = np.where(bad[:, None], np.nan, den[key] / Z[:, None])
            out["cancel_" + key] = np.where(den[key] != 0, ab[key] / np.abs(den[key]), np.inf)
    return out


def worst_cancellation(ref, good=None):
    """the largest cancellation factor over the families `good` (default: those that did not fail) and all entries"""
    ok = ref["failed"] == 0 if good is None else good
    return max(float(np.max(ref[k][ok])) for k in ref if k.startswith("cancel_"))


KEYS = ("d_lambda", "d_mu", "d_multiplier")


def close(got, ref, c, label=""):
    """|got - ref| <= 1e-12 + 1e-10 c |ref| on every derivative both sides carry, the same NaN pattern, failed equal.  Where
    `ref` reports its cancellation factors (reverse), an entry is held to its own factor, which never exceeds the largest
    one c stands for: the bound is 1e-10 of the entry's sum of |terms|."""
    assert np.array_equal(np.asarray(got["failed"]), np.asarray(ref["failed"])), label
    worst = 0.0
    for key in KEYS:
        if key not in ref:
            assert key not in got or key == "d_mu", (label, key)
            continue
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape, (label, key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key)
        ok = ~np.isnan(r)
        if ok.any():
            factor = np.full(r.shape, float(c))
            if "cancel_" + key in ref:
                factor = np.minimum(factor, np.maximum(1.0, ref["cancel_" + key]))
            ratio = np.abs(g[ok] - r[ok]) / (1e-12 + 1e-10 * factor[ok] * np.abs(r[ok]))
            worst = max(worst, float(ratio.max()))
    print("%s: worst |got - ref| / bound (c = %g) = %.3g" % (label, c, worst))
    assert worst <= 1.0, (label, worst)
    return worst
