"""Plain numpy statement of the marginal ancestral reconstruction (a helper, not a test).

The model is the scorer's: leaf vectors one-hot at the observed count (or the error model's taps), interior sizes 0..M,
root sizes 1..R weighted by the float prior, categories mixed with cat_probs.  `updown` runs the up and the down pass of
sum-products; `brute_force` enumerates every assignment of the interior nodes of a tiny problem.  Both take the
transition matrices as an argument: mats[k][v] is the N x N matrix (P[parent size][child size]) of the branch above node
v in category k, None at the root.
"""
import itertools

import numpy as np


def children_of(pb):
    ch = [[] for _ in range(pb.n_nodes)]
    for v in range(pb.n_nodes):
        if pb.parent[v] >= 0:
            ch[int(pb.parent[v])].append(v)
    return ch


def root_of(pb):
    return int(np.where(pb.parent < 0)[0][0])


def oracle_matrices(pb, pr, oracle):
    """mats[k][v] from oracle.build_matrix (which applies the reference's key quantization itself)."""
    mults = [1.0] if pr.multipliers is None else list(pr.multipliers)
    N = pb.matrix_size
    out = []
    for m in mults:
        cache, row = {}, []
        for v in range(pb.n_nodes):
            if pb.parent[v] < 0:
                row.append(None)
                continue
            key = (float(pr.lambdas[pb.lambda_index[v]]) * m, float(pb.branch_length[v]))
            if key not in cache:
                cache[key] = oracle.build_matrix(N, key[0], key[1])
            row.append(cache[key])
        out.append(row)
    return out


def leaf_vector(pb, pr, f, v):
    """The scorer's leaf vector over sizes 0..M (probability.cpp:179-199)."""
    M = pb.max_family_size
    x = int(pb.counts[f, pb.leaf_taxon[v]])
    e = np.zeros(M + 1)
    if pr.error_model is None:
        e[x] = 1.0
        return e
    nd = pr.error_model.shape[1]
    for t in range(nd):
        c = x - (nd - 1) // 2 + t
        if 0 <= c <= M:
            e[c] = pr.error_model[x, t]
    return e


def _summary(post, z, level, first_size=0):
    """post: un-normalised masses of sizes first_size.. ; returns mean, mode, lo, hi and how close the integer choices
    are to a tie (mode: relative gap of the two best masses; lo / hi: |CDF - threshold| at and just before the crossing)."""
    p = post / z
    sizes = np.arange(first_size, first_size + len(p))
    mean = float((sizes * p).sum())
    mode = int(sizes[int(np.argmax(p))])
    cdf = np.cumsum(p)
    out = {"mean": mean, "mode": mode}
    top = np.sort(p)[::-1]
    out["mode_gap"] = float((top[0] - top[1]) / top[0]) if len(top) > 1 and top[0] > 0 else 1.0
    for name, thr in (("lo", 0.5 * (1 - level)), ("hi", 1 - 0.5 * (1 - level))):
        hit = np.where(cdf >= thr)[0]
        idx = int(hit[0]) if len(hit) else len(p) - 1
        out[name] = int(sizes[idx])
        out[name + "_gap"] = float(np.min(np.abs(cdf - thr)))
    return out


MUTANTS = ("split_takes_the_diagonal", "root_range_stops_short", "prior_indexed_at_s")


def updown_family(pb, pr, mats, f, level, detail=False, mutant=None):
    """One family.  Returns a dict: per node arrays mean / mode / lo / hi / p_increase / p_decrease (+ the *_gap tie
    measures), log_evidence, failed, and root_inside[k] = B_root[1..R] (inference_prune's return).

    detail: also Z, post[v] (the un-normalised posterior of node v over sizes 0..max(M, R), categories mixed) and
    row0[v] = (G_v[0], sum_i G_v[i]) with G_v[0] = O[p][0] prod F_sib[0], p the parent of v (categories mixed).
    mutant: one of MUTANTS -- a deliberately WRONG pass, for tests that ask whether their inputs can tell:
    the branch split takes i <= j for i < j; the root takes sizes 1..R-1; the prior is read at s, not s - 1."""
    assert mutant is None or mutant in MUTANTS, mutant
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    ch, root = children_of(pb), root_of(pb)
    K = len(mats)
    probs = [1.0] if pr.cat_probs is None else [float(x) for x in pr.cat_probs]
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)
    post = [np.zeros(max(M, R) + 1) for _ in range(n)]
    inc, dec = np.zeros(n), np.zeros(n)
    root_inside = []
    row0 = np.zeros((n, 2))
    Z = 0.0
    for k in range(K):
        P = mats[k]
        B, F = [None] * n, [None] * n
        for v in range(n):                                   # children before parents
            if pb.leaf_taxon[v] >= 0:
                B[v] = leaf_vector(pb, pr, f, v)
            else:
                top = R if v == root else M
                b = np.ones(top + 1)
                for c in ch[v]:
                    F[c] = P[c][:top + 1, :M + 1] @ B[c]
                    b = b * F[c]
                B[v] = b
        O = [None] * n
        o = np.zeros(R + 1)
        o[1:] = prior[:R]
        if mutant == "root_range_stops_short":
            o[R] = 0.0
        elif mutant == "prior_indexed_at_s":
            o[1:R] = prior[1:R]
            o[R] = 0.0
        O[root] = o
        root_inside.append(B[root][1:R + 1].copy())
        Z += probs[k] * float((O[root] * B[root]).sum())
        post[root][:R + 1] += probs[k] * O[root] * B[root]
        for p in range(n - 1, -1, -1):                       # parents before children
            if pb.leaf_taxon[p] >= 0:
                continue
            top = R if p == root else M
            for v in ch[p]:
                G = O[p].copy()
                for w in ch[p]:
                    if w != v:
                        G = G * F[w]
                Pv = P[v][:top + 1, :M + 1]
                O[v] = G @ Pv
                row0[v] += probs[k] * np.array([G[0], G.sum()])
                post[v][:M + 1] += probs[k] * O[v] * B[v]
                joint = G[:, None] * Pv * B[v][None, :]      # [parent size i][size j]
                i = np.arange(top + 1)[:, None]
                j = np.arange(M + 1)[None, :]
                inc[v] += probs[k] * float(joint[(i <= j) if mutant == "split_takes_the_diagonal" else (i < j)].sum())
                dec[v] += probs[k] * float(joint[i > j].sum())
    res = _finish(pb, pr, f, level, post, inc, dec, Z, root_inside)
    if detail:
        res.update(Z=Z, post=post, row0=row0)
    return res


def _finish(pb, pr, f, level, post, inc, dec, Z, root_inside):
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    root = root_of(pb)
    res = {k: np.full(n, np.nan) for k in ("mean", "p_increase", "p_decrease")}
    res.update({k: np.full(n, -1, dtype=np.int64) for k in ("mode", "lo", "hi")})
    res.update({k: np.ones(n) for k in ("mode_gap", "lo_gap", "hi_gap")})
    res["root_inside"] = root_inside
    res["failed"] = int(not (Z > 0 and np.isfinite(Z)))
    res["log_evidence"] = np.nan if res["failed"] else float(np.log(Z))
    if res["failed"]:
        return res
    for v in range(n):
        if pb.leaf_taxon[v] >= 0 and pr.error_model is None:
            x = int(pb.counts[f, pb.leaf_taxon[v]])
            s = {"mean": float(x), "mode": x, "lo": x, "hi": x, "mode_gap": 1.0, "lo_gap": 1.0, "hi_gap": 1.0}
        elif pb.leaf_taxon[v] >= 0:
            x = int(pb.counts[f, pb.leaf_taxon[v]])
            nd = pr.error_model.shape[1]
            taps = [c for c in range(x - (nd - 1) // 2, x - (nd - 1) // 2 + nd) if 0 <= c <= M]
            s = _summary(post[v][taps[0]:taps[-1] + 1], Z, level, taps[0])
        elif v == root:
            s = _summary(post[v][1:R + 1], Z, level, 1)
        else:
            s = _summary(post[v][:M + 1], Z, level, 0)
        for key, val in s.items():
            res[key][v] = val
        if v != root:
            res["p_increase"][v] = inc[v] / Z
            res["p_decrease"][v] = dec[v] / Z
    return res


def brute_force_family(pb, pr, mats, f, level):
    """The same outputs by enumerating every assignment of the interior nodes (and of the leaves' true sizes under an error
    model): tiny problems only."""
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    root = root_of(pb)
    K = len(mats)
    probs = [1.0] if pr.cat_probs is None else [float(x) for x in pr.cat_probs]
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)
    ranges = []
    leafvec = {}
    for v in range(n):
        if pb.leaf_taxon[v] >= 0:
            leafvec[v] = leaf_vector(pb, pr, f, v)
            ranges.append([c for c in range(M + 1) if leafvec[v][c] != 0.0])
        elif v == root:
            ranges.append(list(range(1, R + 1)))
        else:
            ranges.append(list(range(M + 1)))
    post = [np.zeros(max(M, R) + 1) for _ in range(n)]
    inc, dec = np.zeros(n), np.zeros(n)
    root_inside = [np.zeros(R) for _ in range(K)]
    Z = 0.0
    for k in range(K):
        P = mats[k]
        for assign in itertools.product(*ranges):
            w = 1.0
            for v in range(n):
                if v in leafvec:
                    w *= leafvec[v][assign[v]]
                if v != root:
                    w *= P[v][assign[pb.parent[v]], assign[v]]
                if w == 0.0:
                    break
            if w == 0.0:
                continue
            root_inside[k][assign[root] - 1] += w
            w *= probs[k] * prior[assign[root] - 1]
            Z += w
            for v in range(n):
                post[v][assign[v]] += w
                if v != root:
                    if assign[v] > assign[pb.parent[v]]:
                        inc[v] += w
                    elif assign[v] < assign[pb.parent[v]]:
                        dec[v] += w
    return _finish(pb, pr, f, level, post, inc, dec, Z, root_inside)


KEYS = ("mean", "mode", "lo", "hi", "p_increase", "p_decrease", "mode_gap", "lo_gap", "hi_gap")


def updown(pb, pr, mats, level, families=None, detail=False, mutant=None):
    """All (or the listed) families -> arrays shaped like Context.marginal_reconstruct's, plus the tie measures (and with
    detail: Z [family], post [family][node][size], row0 [family][node][2], see updown_family)."""
    fams = range(pb.n_families) if families is None else families
    rows = [updown_family(pb, pr, mats, f, level, detail=detail, mutant=mutant) for f in fams]
    out = {k: np.stack([r[k] for r in rows]) for k in KEYS}
    out["log_evidence"] = np.array([r["log_evidence"] for r in rows])
    out["failed"] = np.array([r["failed"] for r in rows], dtype=np.int32)
    out["root_inside"] = [r["root_inside"] for r in rows]
    if detail:
        out["Z"] = np.array([r["Z"] for r in rows])
        out["post"] = np.array([r["post"] for r in rows])
        out["row0"] = np.array([r["row0"] for r in rows])
    return out


def excused(ref, tol=1e-9):
    """Boolean masks (mode, lo, hi) of the cells where the reference's own choice is within `tol` of a tie."""
    return ref["mode_gap"] <= tol, ref["lo_gap"] <= tol, ref["hi_gap"] <= tol


def context_matrices(ctx, pb, K):
    """mats[k][v] read back from the device context (the matrices its last call built)."""
    return [[None if pb.parent[v] < 0 else ctx.matrix(v, k) for v in range(pb.n_nodes)] for k in range(K)]
