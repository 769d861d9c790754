"""Plain numpy statement of the transition matrices under separate birth and death rates (a helper, not a test).

The single-lineage law of the linear birth-death process over a branch is p1(0) = alpha, p1(k) = (1-alpha)(1-beta) beta^(k-1);
row s of P is its s-fold convolution.  Three ways to the same matrix, none of them the kernel's:
  closed_form   sum_k C(i,k) C(i+j-k-1, i-1) alpha^(i-k) beta^(j-k) (1-alpha-beta)^k in log space (coeff >= 0: all terms >= 0);
  by_convolve   row s = np.convolve(row s-1, p1), truncated to the order;
  by_filter     the same convolution as a first-order recursive filter (scipy.signal.lfilter): O(N^2), for the large orders.
rates() evaluates alpha and beta from the quantized key with 60-digit decimals, straight from the textbook formula.
kmajor_emulation() writes down what the k-major build does -- the recurrence of the EXCHANGED process, scaled by s/c, with the
two places that are not exchanged -- and lets a caller get each of them wrong on purpose.
"""
import decimal

import numpy as np

import marginal_ref as MR
from cafexp_amd import problem as P
from cafexp_amd.gamma_rates import discrete_gamma


def quantize(lam, mu, t):
    """matrix_cache_key's quantization (matrix_cache.h:42-61), applied to both rates"""
    return int(lam * 1000000000) / 1000000000.0, int(mu * 1000000000) / 1000000000.0, int(t * 1000) / 1000.0


def rates(lam, mu, t):
    """(alpha, beta, zero) of the quantized key, alpha = mu (E-1) / (lambda E - mu), beta = lambda (E-1) / (lambda E - mu),
    E = exp((lambda - mu) t), in 60-digit decimal arithmetic rounded once to double; equal rates: lambda t / (1 + lambda t)."""
    lq, mq, tq = quantize(lam, mu, t)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        L, M, T = decimal.Decimal(lq), decimal.Decimal(mq), decimal.Decimal(tq)
        if L == M:
            a = b = L * T / (1 + L * T)
        else:
            E = ((L - M) * T).exp()
            a, b = M * (E - 1) / (L * E - M), L * (E - 1) / (L * E - M)
        coeff = 1 - a - b
        a, b, coeff = float(a), float(b), float(coeff)
    return a, b, not (coeff > 0 and coeff != 1)


def _row0(n):
    e = np.zeros(n)
    e[0] = 1.0
    return e


def closed_form(n, alpha, beta):
    """P[i][j], i, j < n, from the closed form; needs coeff = 1 - alpha - beta >= 0"""
    from scipy.special import gammaln, logsumexp, xlogy
    coeff = 1.0 - alpha - beta
    assert coeff >= 0
    P = np.zeros((n, n))
    P[0] = _row0(n)
    j = np.arange(n)[:, None]
    k = np.arange(n)[None, :]
    for i in range(1, n):
        with np.errstate(divide="ignore", invalid="ignore"):
            lt = (gammaln(i + 1) - gammaln(k + 1) - gammaln(i - k + 1)                      # C(i, k)
                  + gammaln(i + j - k) - gammaln(i) - gammaln(j - k + 1)                    # C(i+j-k-1, i-1)
                  + xlogy(i - k, alpha) + xlogy(j - k, beta) + xlogy(k, coeff))
        lt = np.where((k <= i) & (k <= j), lt, -np.inf)
        P[i] = np.exp(logsumexp(lt, axis=1))
    return P


def p1(n, alpha, beta):
    p = np.empty(n)
    p[0] = alpha
    p[1:] = (1 - alpha) * (1 - beta) * beta ** np.arange(n - 1)
    return p


def by_convolve(n, alpha, beta):
    one = p1(n, alpha, beta)
    P = np.zeros((n, n))
    P[0] = _row0(n)
    for s in range(1, n):
        P[s] = np.convolve(P[s - 1], one)[:n]
    return P


def by_filter(n, alpha, beta):
    from scipy.signal import lfilter
    q = (1 - alpha) * (1 - beta)
    P = np.zeros((n, n))
    P[0] = _row0(n)
    for s in range(1, n):
        P[s] = alpha * P[s - 1] + q * lfilter([0.0, 1.0], [1.0, -beta], P[s - 1])
    return P


def matrix(n, lam, mu, t, fast=None):
    """The reference matrix of the key (lam, mu, t) with the library's zero rule: rows s >= 1 are 0 for a slot marked zero."""
    a, b, zero = rates(lam, mu, t)
    if zero:
        P = np.zeros((n, n))
        P[0] = _row0(n)
        return P
    return by_filter(n, a, b) if (n > 65 if fast is None else fast) else by_convolve(n, a, b)


def kmajor_emulation(n, alpha, beta, exchange=True, row0_from="alpha", left_from="beta"):
    """P[s][c] as the k-major build produces it: for c >= 1 row c of the process with the rates EXCHANGED (tail ratio alpha,
    extinction beta), scaled by s/c; column 0 (the stored row 0) = alpha^s; the exchanged process's own column 0, which the
    first owned column sees to its left, = beta^(r-1).  exchange=False, row0_from="beta", left_from="alpha": the mistakes."""
    from scipy.signal import lfilter
    outer, tail = (beta, alpha) if exchange else (alpha, beta)
    q = (1 - alpha) * (1 - beta)
    left = {"alpha": alpha, "beta": beta}[left_from]
    first = {"alpha": alpha, "beta": beta}[row0_from]
    s = np.arange(n, dtype=np.float64)
    P = np.zeros((n, n))
    P[0] = _row0(n)
    P[1:, 0] = first ** s[1:]
    row = np.zeros(n)                                # row r-1 of the exchanged process, columns 1 .. n-1 (index 0 unused)
    for r in range(1, n):
        x = np.concatenate(([left ** (r - 1)], row[1:n - 1]))        # what column c sees to its left, c = 1 .. n-1
        row[1:] = outer * row[1:] + q * lfilter([1.0], [1.0, -tail], x)
        P[1:, r] = np.minimum(row[1:] * (s[1:] / r), 1.0)
    return P


def worst_rel(got, want, floor=1e-290):
    """the K1 parity metric (tests/test_gpu_parity.py): largest relative difference over the entries of `want` above the floor"""
    big = want > floor
    return float((np.abs(got - want)[big] / want[big]).max(initial=0.0))


def differs(got, want, tol):
    """True when `got` fails the K1 parity check against `want`: a relative difference above tol where `want` is above 1e-290,
    or an entry above 1e-280 where the other matrix has (nearly) underflowed"""
    big = want > 1e-290
    return bool(worst_rel(got, want) > tol or got[~big].max(initial=0.0) > 1e-280 or want[got <= 1e-290].max(initial=0.0) > 1e-280)


# What the GPU matrix test (tests/test_bd_lm_gpu.py) builds, and what tests/test_bd_lm_model.py shows those inputs can tell apart:
# one order inside each store path and width class of the kernel; rho = lambda/mu in {0.25, 0.8, 1.25, 4}, pure birth, pure death
# (coeff > 0 for all of them), and one saturated pair
ORDERS = (3, 16, 65, 129, 257, 751, 1537, 2048)
RATES = {
    "rho_0.25": (0.004, 0.016, 30.0),
    "rho_0.8": (0.008, 0.010, 30.0),
    "rho_1.25": (0.010, 0.008, 30.0),
    "rho_4": (0.016, 0.004, 30.0),
    "pure_birth": (0.010, 0.0, 30.0),
    "pure_death": (0.0, 0.010, 30.0),
}
SATURATED = (0.05, 0.04, 40.0)
VEC_TOL = 5e-11          # tests/test_gpu_parity.py: K1 against the oracle


# ------------------------------------------------------------------ the context tests' problem and its numpy prune
# six taxa: a cherry (A, B), a trifurcation (C, D, E), a leaf under the root (F), depth 3; two lambda classes
NEWICK = "(((A:3,B:4):2,(C:2,D:2.5,E:3):2.5):3,F:9);"
LAMBDA_TREE = "(((A:1,B:1):1,(C:2,D:2,E:2):2):1,F:2);"
SPECIES = ["A", "B", "C", "D", "E", "F"]
LAMBDAS = np.array([0.012, 0.006])
MUS = np.array([0.007, 0.009])
SHAPES = {41: (40, 30, [1, 2, 3, 5, 8, 12, 20, 30]), 300: (299, 250, [1, 3, 8, 20, 45, 90, 150, 220])}


def problem(order, n_dev=0):
    M, Rr, base = SHAPES[order]
    rng = np.random.default_rng(order)
    counts = np.clip(np.array(base)[:, None] + rng.integers(-2, 4, size=(8, 6)), 0, M - 2).astype(np.int32)
    pb = P.build_problem(P.parse_newick(NEWICK), SPECIES, ["f%d" % i for i in range(8)], counts,
                         lambda_tree=P.parse_newick(LAMBDA_TREE, lambda_tree=True), root_filter=False,
                         max_family_size=M, max_root_family_size=Rr, n_deviations=n_dev)
    assert pb.matrix_size == order and pb.n_lambdas == 2 and not pb.single_lambda
    return pb


def params(pb, model):
    pr = P.Params(lambdas=LAMBDAS.copy(), prior=P.prior_uniform(pb.max_root_family_size))
    if model == "gamma":
        pr.cat_probs, pr.multipliers = discrete_gamma(3, 0.7)
    if model == "error":
        em = np.tile(np.array([0.05, 0.9, 0.05]), (pb.max_family_size + 1, 1))
        em[0] = [0.0, 0.95, 0.05]
        pr.error_model = em
    return pr


def reference_matrices(pb, lambdas, mus, mults):
    N, cache, out = pb.matrix_size, {}, []
    for m in mults:
        row = []
        for v in range(pb.n_nodes):
            if pb.parent[v] < 0:
                row.append(None)
                continue
            i = pb.lambda_index[v]
            key = (float(lambdas[i]) * m, float(mus[i]) * m, float(pb.branch_length[v]))
            if key not in cache:
                cache[key] = matrix(N, *key)
            row.append(cache[key])
        out.append(row)
    return out


def score_from_root_vectors(pr, inside):
    """inside[f][k] = B_root[1..R]; the scorer's reduction (base_model.cpp:89-105, gamma_core.cpp:144-216)"""
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)
    total = 0.0
    for fam in inside:
        if pr.multipliers is None:
            with np.errstate(divide="ignore"):
                total += np.max(np.log(fam[0]) + np.log(prior))
        else:
            total += np.log(sum(p * np.max(v * prior) for p, v in zip(pr.cat_probs, fam)))
    return -total


def pupko(pb, mats, root_prior, f):
    """gene_family_reconstructor.cpp:13-165 in numpy on the given matrices"""
    n, M, Rr = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    ch, root = MR.children_of(pb), MR.root_of(pb)
    L, Cc = np.zeros((n, M + 1)), np.zeros((n, M + 1), dtype=np.int64)
    for v in range(n):
        if pb.leaf_taxon[v] >= 0:
            x = int(pb.counts[f, pb.leaf_taxon[v]])
            L[v, 1:] = mats[v][1:M + 1, x]
            Cc[v] = x
            continue
        value = np.ones(M + 1)
        for u in ch[v]:
            value = value * L[u]
        if v == root:
            lr = min(M, Rr) + 1
            val = value[1:lr] * np.asarray(root_prior, dtype=np.float32).astype(np.float64)[1:lr]
            Cc[v, 0] = 1 + int(np.argmax(val)) if val.max() > -1 else 0
            continue
        val = mats[v][:M + 1, :M + 1] * value[None, :]
        Cc[v] = np.argmax(val, axis=1)                   # first maximum, as the strict > of the scan
        L[v] = val.max(axis=1)
    state = np.zeros(n, dtype=np.int32)
    state[root] = Cc[root, 0]
    for v in range(n - 1, -1, -1):
        if v != root:
            state[v] = Cc[v, state[pb.parent[v]]]
    return state
