"""Plain numpy statement of the gene-gain model (a helper, not a test): the linear birth-death process with immigration,
n -> n+1 at rate n lambda + nu, n -> n-1 at rate n mu.

Row 0 of the transition matrix is the law of the immigrants' descendants, negative binomial with r = nu / lambda and the beta
of the single-lineage law (Poisson for lambda = 0), written with scipy's gammaln; row s is row s-1 convolved with the
single-lineage law p1 of tests/bd_lm_ref.py.  generator() is the truncated rate matrix whose expm the closed form is checked
against.  prune() is a small sum-product over root sizes 0..R that owes nothing to the library: the root has mass root_absent
at size 0 and (1 - root_absent) prior[j-1] at size j.  Every function takes a `wrong` switch that gets the model wrong on purpose
(tests/test_gain_model.py shows that the test tables tell each from the right one)."""
import numpy as np

import bd_lm_ref as R
import marginal_ref as MR

WRONG = ("nu_ignored", "r_over_mu", "alpha_in_row0", "row0_everywhere")


def quantize(x):
    return int(x * 1000000000) / 1000000000.0


def row0(n, lam, mu, nu, t, wrong=None):
    """P[0][0..n-1] of the quantized key"""
    from scipy.special import gammaln
    lq, mq, tq = R.quantize(lam, mu, t)
    nq = quantize(nu)
    k = np.arange(n, dtype=np.float64)
    e0 = np.zeros(n)
    e0[0] = 1.0
    if nq == 0 or wrong == "nu_ignored":
        return e0
    if lq == 0:
        m = nq * tq if mq == 0 else nq * -np.expm1(-mq * tq) / mq
        if m == 0:
            return e0
        return np.exp(-m + k * np.log(m) - gammaln(k + 1))
    a, b, _ = R.rates(lam, mu, t)
    if wrong == "alpha_in_row0":
        b = a
    if b == 0:
        return e0
    r = nq / (mq if wrong == "r_over_mu" else lq)
    return np.exp(gammaln(r + k) - gammaln(r) - gammaln(k + 1) + r * np.log1p(-b) + k * np.log(b))


def matrix(n, lam, mu, nu, t, wrong=None):
    """The matrix of the key (lam, mu, nu, t) with the library's zero rule: a key marked zero has rows s >= 1 all 0."""
    from scipy.signal import lfilter
    a, b, zero = R.rates(lam, mu, t)
    P = np.zeros((n, n))
    P[0] = row0(n, lam, mu, nu, t, wrong)
    if zero:
        return P
    q = (1 - a) * (1 - b)
    for s in range(1, n):
        if n > 65:
            P[s] = a * P[s - 1] + q * lfilter([0.0, 1.0], [1.0, -b], P[s - 1])
        else:
            P[s] = np.convolve(P[s - 1], R.p1(n, a, b))[:n]
        if wrong == "row0_everywhere":                     # the immigrants' law convolved in again at every row step
            P[s] = np.convolve(P[s], P[0])[:n]
    return P


def generator(n, lam, mu, nu):
    """Rate matrix of the process on sizes 0..n-1 (the last size keeps its outflow: mass leaves the truncation)"""
    Q = np.zeros((n, n))
    for i in range(n):
        up, down = i * lam + nu, i * mu
        if i + 1 < n:
            Q[i, i + 1] = up
        if i > 0:
            Q[i, i - 1] = down
        Q[i, i] = -(up + down)
    return Q


def matrices(pb, lambdas, mus, nus, wrong=None):
    """mats[v] of every branch (None at the root) at order pb.matrix_size"""
    cache, out = {}, []
    for v in range(pb.n_nodes):
        if pb.parent[v] < 0:
            out.append(None)
            continue
        i = pb.lambda_index[v]
        key = (float(lambdas[i]), float(mus[i]), float(nus[i]), float(pb.branch_length[v]))
        if key not in cache:
            cache[key] = matrix(pb.matrix_size, *key, wrong=wrong)
        out.append(cache[key])
    return out


def leaf_vector(pb, error_model, counts, v):
    """likelihood of sizes 0..M at leaf v; a missing cell (count < 0) is all ones"""
    M = pb.max_family_size
    x = int(counts[pb.leaf_taxon[v]])
    if x < 0:
        return np.ones(M + 1)
    e = np.zeros(M + 1)
    if error_model is None:
        e[x] = 1.0
        return e
    nd = error_model.shape[1]
    for t in range(nd):
        c = x - (nd - 1) // 2 + t
        if 0 <= c <= M:
            e[c] = error_model[x, t]
    return e


def root_likelihoods(pb, counts, mats, error_model=None):
    """L[0..R]: the likelihood of the leaf counts for every root size"""
    M, Rr = pb.max_family_size, pb.max_root_family_size
    ch, root = MR.children_of(pb), MR.root_of(pb)
    order, stack = [], [root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(ch[v])
    factor = {}
    for v in reversed(order):
        if v == root:
            continue
        vec = leaf_vector(pb, error_model, counts, v) if pb.leaf_taxon[v] >= 0 else np.prod([factor[u][:M + 1] for u in ch[v]], axis=0)
        rows = (Rr if pb.parent[v] == root else M) + 1
        factor[v] = mats[v][:rows, :M + 1] @ vec
    return np.prod([factor[u][:Rr + 1] for u in ch[root]], axis=0)


def reduce_root(L, prior, root_absent, rule):
    """lnL from L[0..R]: mass root_absent at size 0, (1 - root_absent) (double)(float)prior[j-1] at size j; rule "max" or "sum" """
    from scipy.special import logsumexp
    mass = np.concatenate([[root_absent], (1.0 - root_absent) * np.asarray(prior, dtype=np.float32).astype(np.float64)[:len(L) - 1]])
    with np.errstate(divide="ignore"):
        t = np.log(L) + np.log(mass)
    return np.max(t) if rule == "max" else logsumexp(t)


def root_vectors(pb, lambdas, mus, nus, families=None, error_model=None, wrong=None):
    """L[i][0..R] of family families[i] (an index, or -1 for the all-zero profile) under row i of lambdas / mus / nus [n][n_lambdas]"""
    families = np.arange(pb.n_families) if families is None else np.asarray(families)
    lam, mu, nu = (np.asarray(x, dtype=np.float64).reshape(len(families), -1) for x in (lambdas, mus, nus))
    out, cache = [], {}
    for i, f in enumerate(families):
        key = (tuple(lam[i]), tuple(mu[i]), tuple(nu[i]))
        if key not in cache:
            cache[key] = matrices(pb, lam[i], mu[i], nu[i], wrong=wrong)
        counts = np.zeros(pb.n_taxa, dtype=np.int64) if f < 0 else pb.counts[f]
        out.append(root_likelihoods(pb, counts, cache[key], error_model))
    return out


def prune(pb, prior, lambdas, mus, nus, root_absent, rule, families=None, error_model=None, wrong=None):
    """lnL per listed family: root_vectors reduced by reduce_root"""
    return np.array([reduce_root(L, prior, root_absent, rule) for L in root_vectors(pb, lambdas, mus, nus, families, error_model, wrong)])


# What tests/test_gain_gpu.py runs on the three-taxon tree of tests/test_per_family_shapes.py, one (lambda, mu, nu) per family:
# lambda / mu = 0.25, 0.8, 1.25, 4 (tests/test_per_family_lm.py), nu / lambda = 0.5, 1.5, 0.2, 1
RATES3 = np.array([(0.0011, 0.0044, 0.00055), (0.002, 0.0025, 0.003), (0.0051, 0.00408, 0.00102), (0.0034, 0.00085, 0.0034)])
