"""Plain numpy statements of the per-branch log-rate scores of cafe_branch_scores and of the rate-shift score test built on
them (a helper, not a test).  gradient_ref is imported as it stands.

The score: for a family f and the branch above node v, with c_v a factor on the rates of that branch alone,
    rate[f][v] = d log Z_f / d log c_v at c = 1      (both rates), birth / death: a factor on lambda / on mu alone.
Two routes, neither of them the kernels':
  complex_step   gradient_ref's complex prune with the imaginary part 1e-30 * (lambda_q m_k, mu_q m_k) on the rates of ONE
                 branch in every category: Im(log Z) / 1e-30, no subtraction;
  reverse        the reverse-mode contraction G_v^T (dP_v / d theta) B_v of gradient_ref.reverse, kept per branch instead
                 of added per lambda index, each category weighted p_k m_k lambda_q (or mu_q); with every entry's
                 cancellation factor sum |terms| / |sum terms| (cancel_<name>).  `mutant` makes one deliberately WRONG pass.
The rates are quantized like the library's keys and the derivative is that of the smooth likelihood at the quantized point,
as in gradient_ref; the factor lambda_q m_k in front is the unquantized one, so that the scores of the branches of one lambda
index add up to lambda_q d_lambda_q.

The statistic (score_test, holm, clade_directions): Rao's efficient score for a direction a in branch-score space, the
searched global parameters profiled out through the Gram matrix of the per-family score vectors.
"""
import math

import numpy as np

import gradient_ref as GR
import marginal_ref as MR

STEP = GR.STEP
MUTANTS = ("slot_from_lambda_index", "mu_dropped", "multiplier_dropped")
NAMES = ("rate", "birth", "death")


def _rates(pb, pr, mus):
    lam = np.asarray(pr.lambdas, dtype=float)
    return lam, (lam if mus is None else np.asarray(mus, dtype=float))


def log_z(pb, pr, mus, rule, leafv, branch=None, kind="rate", args=None):
    """gradient_ref.log_z with the step on one branch: node `branch` gets lambda_q m_k (kind rate / birth) and mu_q m_k (rate /
    death) times 1e-30 on the imaginary axis of its rates in every category"""
    n, N = pb.n_nodes, pb.matrix_size
    root = MR.root_of(pb)
    lam, mu = _rates(pb, pr, mus)
    use_log = pr.multipliers is None and rule == "max"
    z, lbest = 0.0, None
    for k, (m, p) in enumerate(zip(GR._mults(pr), GR._probs(pr))):
        keys, cache, P = GR.branch_keys(pb, pr, mus, k), {}, [None] * n
        for v in range(n):
            if keys[v] is None:
                continue
            lq, mq, tq = keys[v]
            q = int(pb.lambda_index[v])
            dl = lam[q] * m if v == branch and kind in ("rate", "birth") else 0.0
            dm = mu[q] * m if v == branch and kind in ("rate", "death") else 0.0
            key = (lq, mq, tq, dl, dm)
            if key not in cache:
                a0, b0 = GR.alpha_beta(lq, mq, tq)
                a, b = GR.alpha_beta(lq + 1j * STEP * dl, mq + 1j * STEP * dm, tq)
                cache[key] = GR.matrix(N, a, b, GR.is_zero(a0, b0))
            P[v] = cache[key]
        B, _ = GR._up(pb, P, leafv, complex)
        O, arg = GR._root_weight(pb, pr, B[root], rule, use_log)
        if args is not None:
            args.append(arg)
        zk = (O * B[root]).sum(axis=0)
        z = z + p * zk
        if use_log:
            lbest = np.log(zk)
    with np.errstate(divide="ignore", invalid="ignore"):
        return lbest if use_log else np.log(z)


def complex_step(pb, pr, mus=None, rule="max"):
    """dict: family_lnl, failed, rate [F][n_nodes] (NaN at the root), birth and death with mus"""
    leafv = GR.leaf_vectors(pb, pr)
    base = log_z(pb, pr, mus, rule, leafv)
    F, n = pb.n_families, pb.n_nodes
    out = {"family_lnl": base.real.copy(), "failed": (~np.isfinite(base.real)).astype(np.int32)}
    for kind in NAMES if mus is not None else NAMES[:1]:
        out[kind] = np.full((F, n), np.nan)
        for v in range(n):
            if pb.parent[v] >= 0:
                out[kind][:, v] = log_z(pb, pr, mus, rule, leafv, branch=v, kind=kind).imag / STEP
        out[kind][out["failed"] == 1] = np.nan
    return out


def reverse(pb, pr, mus=None, rule="max", mutant=None):
    """gradient_ref.reverse's dict (the global scores with their factors) plus rate, birth, death [F][n_nodes] and
    cancel_rate, cancel_birth, cancel_death (inf where the sum of the terms is 0)."""
    assert mutant is None or mutant in MUTANTS, mutant
    out = GR.reverse(pb, pr, mus, rule)
    n, M, R, N, F = pb.n_nodes, pb.max_family_size, pb.max_root_family_size, pb.matrix_size, pb.n_families
    ch, root = MR.children_of(pb), MR.root_of(pb)
    leafv = GR.leaf_vectors(pb, pr)
    mults, probs = GR._mults(pr), GR._probs(pr)
    lam, mu = _rates(pb, pr, mus)
    n_par = 1 if mus is None else 2
    use_log = pr.multipliers is None and rule == "max"
    val, ab = np.zeros((n_par, n, F)), np.zeros((n_par, n, F))
    Z = np.zeros(F)
    steps = [(1.0, 1.0)] if mus is None else [(1.0, 0.0), (0.0, 1.0)]
    if mus is None and mutant == "mu_dropped":
        steps = [(1.0, 0.0)]
    for k in range(len(mults)):
        keys, P, rates, cache = GR.branch_keys(pb, pr, mus, k), [None] * n, [None] * n, {}
        for v in range(n):
            if keys[v] is None:
                continue
            lq, mq, tq = keys[v]
            if keys[v] not in cache:
                a, b = GR.alpha_beta(lq, mq, tq)
                d = []
                for dl, dm in steps:
                    a1, b1 = GR.alpha_beta(lq + 1j * STEP * dl, mq + 1j * STEP * dm, tq)
                    d.append((a1.imag / STEP, b1.imag / STEP))
                cache[keys[v]] = (GR.matrix(N, a, b, GR.is_zero(a, b)).real, (a.real, b.real, GR.is_zero(a, b), d))
            P[v], rates[v] = cache[keys[v]]
        B, Fp = GR._up(pb, P, leafv, float)
        O = [None] * n
        O[root], _ = GR._root_weight(pb, pr, B[root], rule, use_log)
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
                Pv = P[v][:top + 1, :M + 1]
                if pb.leaf_taxon[v] < 0:
                    O[v] = Pv.T @ G
                a, b, zero, d = rates[v]
                if zero:
                    continue
                q = int(pb.lambda_index[v])
                i = np.arange(top + 1)[:, None]
                for t, (da, db) in enumerate(d):
                    coef = probs[k] * (1.0 if mutant == "multiplier_dropped" else mults[k]) * (lam[q] if t == 0 else mu[q])
                    Ft = Pv @ GR.scanned(B[v], a, b, da, db)
                    dP = GR.dense_derivative(Pv, a, b, da, db)
                    slot = q if mutant == "slot_from_lambda_index" else v
                    val[t, slot] += coef * (i[1:] * G[1:] * Ft[:-1]).sum(axis=0)
                    ab[t, slot] += abs(coef) * (np.abs(G) * (np.abs(dP) @ np.abs(B[v]))).sum(axis=0)
    if mus is not None and mutant == "mu_dropped":
        val[1], ab[1] = 0.0, 0.0
    bad = ~((Z > 0) & np.isfinite(Z))
    assert np.array_equal(bad.astype(np.int32), out["failed"])
    nonroot = np.array([pb.parent[v] >= 0 for v in range(n)])

    def put(name, v, a):
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(bad[None, :], np.nan, v / Z[None, :]).T.copy()
            c = np.where(v != 0, a / np.abs(v), np.inf).T.copy()
        x[:, ~nonroot] = np.nan
        c[:, ~nonroot] = np.inf
        out[name], out["cancel_" + name] = x, c
    put("rate", val.sum(axis=0), ab.sum(axis=0))
    if mus is not None:
        put("birth", val[0], ab[0])
        put("death", val[1], ab[1])
    return out


def as_gradient(d):
    """the per-branch arrays under the names gradient_ref.close compares (rate as d_lambda, birth / death as d_multiplier / d_mu),
    so that its bound -- every entry held to its own cancellation factor -- applies as it stands"""
    names = {"rate": "d_lambda", "death": "d_mu", "birth": "d_multiplier"}
    out = {"failed": d["failed"]}
    for mine, theirs in names.items():
        if mine in d:
            out[theirs] = d[mine]
            if "cancel_" + mine in d:
                out["cancel_" + theirs] = d["cancel_" + mine]
    return out


def worst_cancellation(ref):
    ok = ref["failed"] == 0
    nonroot = np.isfinite(ref["cancel_rate"]).any(axis=0)
    return max(float(np.max(ref["cancel_" + k][ok][:, nonroot])) for k in NAMES if "cancel_" + k in ref)


# ------------------------------------------------------------------------------------------------------- the score vector
def score_vectors(res, pb, n_par):
    """z_f [F][P] in the library's order from a result dict (the library's or reverse's): the branch scores of the non-root
    nodes (rate, or birth then death), d_lambda, d_mu, d_multiplier"""
    nonroot = [v for v in range(pb.n_nodes) if pb.parent[v] >= 0]
    cols = [res["rate"][:, nonroot]] if n_par == 1 else [res["birth"][:, nonroot], res["death"][:, nonroot]]
    cols.append(res["d_lambda"])
    if n_par == 2:
        cols.append(res["d_mu"])
    if "d_multiplier" in res:
        cols.append(res["d_multiplier"])
    return np.concatenate(cols, axis=1)


def gram_of(z, failed):
    """(total, gram, |z|^T |z|, n_used) over the families that did not fail, in extended precision"""
    zz = z[np.asarray(failed) == 0].astype(np.longdouble)
    return zz.sum(axis=0), zz.T @ zz, np.abs(zz).T @ np.abs(zz), len(zz)


# ------------------------------------------------------------------------------------------------------- the score test
def subtree(pb, v):
    ch = MR.children_of(pb)
    out, todo = [], [v]
    while todo:
        x = todo.pop()
        out.append(x)
        todo.extend(ch[x])
    return sorted(out)


def directions(pb, n_par, P):
    """per non-root node v: (branch direction, clade direction) in score space [P]: 1 on the joint-rate entries (birth and
    death under death rates) of the branch above v / of every branch of the subtree below and including it"""
    nonroot = [v for v in range(pb.n_nodes) if pb.parent[v] >= 0]
    slot = {v: i for i, v in enumerate(nonroot)}
    nb = len(nonroot)
    out = {}
    for v in nonroot:
        a, c = np.zeros(P), np.zeros(P)
        for p in range(n_par):
            a[p * nb + slot[v]] = 1.0
            for x in subtree(pb, v):
                c[p * nb + slot[x]] = 1.0
        out[v] = (a, c)
    return out


def score_test(total, gram, A, T):
    """A [P][d]: the directions tested jointly (d = 1: one column); T [P][n_theta]: the searched global parameters as
    directions in score space.  Returns dict U [d], V [d][d], stat, p, testable, multiplier (d = 1: exp(U / V)).
    U_a = a^T U - a^T G T (T^T G T)^-1 T^T U,  V_a = a^T G a - a^T G T (T^T G T)^-1 T^T G a,  stat = U^T V^-1 U."""
    A = np.asarray(A, dtype=float).reshape(len(total), -1)
    Ub, Ut = A.T @ total, T.T @ total
    Gbb, Gbt, Gtt = A.T @ gram @ A, A.T @ gram @ T, T.T @ gram @ T
    X = np.linalg.solve(Gtt, np.column_stack([Ut, Gbt.T])) if T.shape[1] else np.zeros((0, 1 + A.shape[1]))
    U = Ub - Gbt @ X[:, 0]
    V = Gbb - Gbt @ X[:, 1:]
    d = A.shape[1]
    ok = bool(np.all(np.diag(V) > 1e-12 * np.diag(Gbb))) and (d == 1 or np.linalg.det(V) > 1e-12 * np.prod(np.diag(Gbb)))
    if not ok:
        return {"U": U, "V": V, "stat": math.nan, "p": math.nan, "testable": False, "multiplier": math.nan}
    stat = float(U @ np.linalg.solve(V, U))
    p = math.erfc(math.sqrt(stat / 2)) if d == 1 else math.exp(-stat / 2)
    return {"U": U, "V": V, "stat": stat, "p": p, "testable": True, "multiplier": math.exp(U[0] / V[0, 0]) if d == 1 else math.nan}


def holm(p):
    """Holm's step-down adjustment over the finite entries; NaN stays"""
    p = np.asarray(p, dtype=float)
    out = np.full(p.shape, np.nan)
    idx = [i for i in np.argsort(p, kind="stable") if np.isfinite(p[i])]
    m, run = len(idx), 0.0
    for rank, i in enumerate(idx):
        run = max(run, min(1.0, (m - rank) * p[i]))
        out[i] = run
    return out


# ------------------------------------------------------------------------------------------- a planted shift (CPU tests)
PLANTED_TREE = "(((A:6,B:6):4,(C:5,D:5):5):5,((E:4,F:4):6,(G:7,H:7):3):5);"
PLANTED_SPECIES = list("ABCDEFGH")
PLANTED_CLADE = ("E", "F")                                   # the cherry (E, F) and the branch above it turn over 4 x as fast
PLANTED_M = 40


def simulate(pb, lambdas_per_node, n, rng, root_sizes=(2, 3, 4, 5, 6)):
    """n families down the tree of pb: the root size uniform over root_sizes, every child from its parent's row of the
    lambda = mu transition matrix of its branch cut at PLANTED_M (the cut-off mass redrawn) -> counts [n][taxa]"""
    N = PLANTED_M + 1
    ch, root = MR.children_of(pb), MR.root_of(pb)
    mats = {}
    for v in range(pb.n_nodes):
        if v != root:
            a, b = GR.alpha_beta(lambdas_per_node[v], lambdas_per_node[v], float(pb.branch_length[v]))
            mats[v] = GR.matrix(N, a, b, False).real
    counts = np.zeros((n, pb.n_taxa), dtype=np.int32)
    for f in range(n):
        size = {root: int(rng.choice(root_sizes))}
        todo = [root]
        while todo:
            p = todo.pop()
            for v in ch[p]:
                row = np.maximum(mats[v][size[p]], 0.0)
                size[v] = int(rng.choice(N, p=row / row.sum()))
                todo.append(v)
        for v in range(pb.n_nodes):
            if pb.leaf_taxon[v] >= 0:
                counts[f, pb.leaf_taxon[v]] = size[v]
    return counts


def planted_problem(counts, lambda_tree=None):
    from cafexp_amd import problem as P
    return P.build_problem(P.parse_newick(PLANTED_TREE), PLANTED_SPECIES, ["f%d" % i for i in range(len(counts))], counts,
                           lambda_tree=None if lambda_tree is None else P.parse_newick(lambda_tree, lambda_tree=True), root_filter=False,
                           max_family_size=PLANTED_M, max_root_family_size=20)


def planted_nodes(pb):
    """the nodes of the planted clade: the subtree below and including the parent of PLANTED_CLADE's leaves"""
    leaves = [v for v in range(pb.n_nodes) if pb.leaf_taxon[v] >= 0 and PLANTED_SPECIES[pb.leaf_taxon[v]] in PLANTED_CLADE]
    top = int(pb.parent[leaves[0]])
    assert all(pb.parent[v] == top for v in leaves)
    return top, subtree(pb, top)


def planted_counts(seed, factor, n=300, lam=0.01):
    from cafexp_amd import problem as P
    pb = planted_problem(np.ones((1, len(PLANTED_SPECIES)), dtype=np.int32))
    rates = np.full(pb.n_nodes, lam)
    rates[planted_nodes(pb)[1]] *= factor
    return simulate(pb, rates, n, np.random.default_rng(seed))


def total_lnl(pb, lambdas, rule="sum"):
    from cafexp_amd import problem as P
    pr = P.Params(lambdas=np.asarray(lambdas, dtype=float), prior=P.prior_uniform(pb.max_root_family_size))
    return float(np.sum(log_z(pb, pr, None, rule, GR.leaf_vectors(pb, pr)).real))


def golden_max(f, lo, hi, iters=40):
    """the maximiser of a unimodal f on [lo, hi] by golden-section search"""
    g = (math.sqrt(5) - 1) / 2
    a, b = lo, hi
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(iters):
        if fc > fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = f(d)
    return (a + b) / 2


def planted_scan(counts, rule="sum"):
    """fit lambda on the reference lnL, then the score tests of every branch and clade at the fit -> dict: lam, lnl, nodes,
    branch / clade (lists of score_test results), branch_holm / clade_holm"""
    from cafexp_amd import problem as P
    pb = planted_problem(counts)
    lam = golden_max(lambda x: total_lnl(pb, [x], rule), 0.002, 0.05)
    pr = P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(pb.max_root_family_size))
    ref = reverse(pb, pr, None, rule)
    z = score_vectors(ref, pb, 1)
    total, gram, _, _ = gram_of(z, ref["failed"])
    total, gram = total.astype(float), gram.astype(float)
    T = np.zeros((z.shape[1], 1))
    T[pb.n_nodes - 1, 0] = 1.0                               # lambda, as it was searched
    dirs = directions(pb, 1, z.shape[1])
    nodes = sorted(dirs)
    out = {"pb": pb, "lam": lam, "lnl": total_lnl(pb, [lam], rule), "nodes": nodes, "total": total}
    for i, kind in enumerate(("branch", "clade")):
        out[kind] = [score_test(total, gram, dirs[v][i], T) for v in nodes]
        out[kind + "_holm"] = holm([t["p"] for t in out[kind]])
    return out
