"""Plain numpy statement of cafe_branch_change (a helper, not a test): the posterior of Delta = size(v) - size(parent(v)) on
the branch above every non-root node, in a band of +-D with both tails.

The model and the passes are tests/marginal_ref.py's (mats[k][v] is the N x N matrix P[parent size][child size] of the
branch above node v in category k, None at the root).  For every branch the joint J[i][j] = G_v[i] P_v[i][j] B_v[j] is formed
explicitly (a leaf's B_v is the scorer's leaf vector: one-hot at the observed count, or the error model's weights at the
true sizes its taps reach) and every one of its diagonals is summed; the band of a given D is cut from those sums, the tails
are the sums of the diagonals beyond it.  `diagonals` (the pass, independent of D) and `summarise` (one D and level) are
separate so that a test computes the pass once.  `brute_force_family` enumerates every assignment of a tiny problem instead.

MUTANTS are deliberately WRONG variants, for tests that ask whether their inputs can tell."""
import itertools

import numpy as np

import marginal_ref as MR

NONE = -(1 << 31)            # CAFE_CHANGE_NONE
MUTANTS = ("d_is_i_minus_j", "row0_dropped", "tail_mask_takes_the_edge", "tap_offset_ignored")


def _summary(band, below, above, z, level):
    """band: un-normalised w[-D..D]; -> mode (first arg max over the band), lo, hi on the CDF over (below, band, above), with
    -D-1 / D+1 for a crossing in a tail, and how close each integer is to a tie."""
    D = (len(band) - 1) // 2
    p = band / z
    out = {"mode": int(np.argmax(p)) - D}
    top = np.sort(p)[::-1]
    out["mode_gap"] = float((top[0] - top[1]) / top[0]) if len(top) > 1 and top[0] > 0 else 1.0
    cdf = np.cumsum(np.concatenate([[below / z], p, [above / z]]))
    for name, thr in (("lo", 0.5 * (1 - level)), ("hi", 1 - 0.5 * (1 - level))):
        hit = np.where(cdf >= thr)[0]
        idx = int(hit[0]) if len(hit) else len(cdf) - 1
        out[name] = idx - 1 - D                              # 0 -> -D - 1 (the lower tail), 2 D + 2 -> D + 1 (the upper)
        out[name + "_gap"] = float(np.min(np.abs(cdf - thr)))
    return out


def _diagonal_sums(J, top, mutant):
    """out[d + top] = sum_i J[i][i + d], d = -top..top (d = j - i)."""
    if mutant == "row0_dropped":
        J = J.copy()
        J[0, :] = 0.0
    i = np.arange(J.shape[0])[:, None]
    j = np.arange(J.shape[1])[None, :]
    d = (i - j) if mutant == "d_is_i_minus_j" else (j - i)
    return np.bincount((d + top).ravel(), weights=J.ravel(), minlength=2 * top + 1)


def _leaf_joint_without_tap_offset(pb, pr, f, v, G, Pv):
    """The wrong leaf joint: every tap's mass booked at the OBSERVED count x instead of the tap's true size c."""
    x = int(pb.counts[f, pb.leaf_taxon[v]])
    e = MR.leaf_vector(pb, pr, f, v)
    J = np.zeros((len(G), pb.max_family_size + 1))
    J[:, x] = (G[:, None] * Pv * e[None, :]).sum(axis=1)
    return J


def diagonals_family(pb, pr, mats, f, mutant=None):
    """One family's pass -> {"full": [n][2 top + 1] un-normalised mass of every d = -top..top (top = max(M, R)), "post": the
    un-normalised posterior of every node's size, "Z"}."""
    assert mutant is None or mutant in MUTANTS, mutant
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    ch, root = MR.children_of(pb), MR.root_of(pb)
    probs = [1.0] if pr.cat_probs is None else [float(x) for x in pr.cat_probs]
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)
    top_d = max(M, R)
    post = np.zeros((n, top_d + 1))
    full = np.zeros((n, 2 * top_d + 1))
    Z = 0.0
    for k in range(len(mats)):
        P = mats[k]
        B, F = [None] * n, [None] * n
        for v in range(n):                                   # children before parents
            if pb.leaf_taxon[v] >= 0:
                B[v] = MR.leaf_vector(pb, pr, f, v)
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
        O[root] = o
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
                post[v][:M + 1] += probs[k] * O[v] * B[v]
                J = G[:, None] * Pv * B[v][None, :]          # [parent size i][size j]
                if mutant == "tap_offset_ignored" and pb.leaf_taxon[v] >= 0 and pr.error_model is not None:
                    J = _leaf_joint_without_tap_offset(pb, pr, f, v, G, Pv)
                full[v] += probs[k] * _diagonal_sums(J, top_d, mutant)
    return {"full": full, "post": post, "Z": Z}


def summarise_family(pb, state, D, level, mutant=None):
    """One family's outputs for one D and level from its pass: per-node arrays pmf [n][2D+1], below, above, mean, mode, lo, hi
    (+ the *_gap tie measures, node_mean -- the posterior mean size of every node -- and mean_scale), log_evidence, failed."""
    n, top = pb.n_nodes, max(pb.max_family_size, pb.max_root_family_size)
    root = MR.root_of(pb)
    full, post, Z = state["full"], state["post"], state["Z"]
    res = {"pmf": np.full((n, 2 * D + 1), np.nan)}
    res.update({k: np.full(n, np.nan) for k in ("below", "above", "mean")})
    res.update({k: np.full(n, NONE, dtype=np.int64) for k in ("mode", "lo", "hi")})
    res.update({k: np.ones(n) for k in ("mode_gap", "lo_gap", "hi_gap")})
    res["failed"] = int(not (Z > 0 and np.isfinite(Z)))
    res["log_evidence"] = np.nan if res["failed"] else float(np.log(Z))
    res["node_mean"] = np.full(n, np.nan)
    res["mean_scale"] = np.ones(n)                           # max(1, the larger of the two node means): what mean is judged on
    if res["failed"]:
        return res
    res["node_mean"] = (post * np.arange(top + 1)[None, :]).sum(axis=1) / Z
    edge = 1 if mutant == "tail_mask_takes_the_edge" else 0  # the wrong tails take |d| = D as well
    for v in range(n):
        if v == root:
            continue
        band = full[v][top - D:top + D + 1]
        below, above = float(full[v][:top - D + edge].sum()), float(full[v][top + D + 1 - edge:].sum())
        res["pmf"][v] = band / Z
        res["below"][v] = below / Z
        res["above"][v] = above / Z
        p = int(pb.parent[v])
        res["mean"][v] = res["node_mean"][v] - res["node_mean"][p]
        res["mean_scale"][v] = max(1.0, res["node_mean"][v], res["node_mean"][p])
        for key, val in _summary(band, below, above, Z, level).items():
            res[key][v] = val
    return res


def change_family(pb, pr, mats, f, D, level, mutant=None):
    return summarise_family(pb, diagonals_family(pb, pr, mats, f, mutant), D, level, mutant)


def brute_force_family(pb, pr, mats, f, D, level):
    """The same outputs by enumerating every assignment of the interior nodes (and of the leaves' true sizes under an error
    model): tiny problems only."""
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    root = MR.root_of(pb)
    probs = [1.0] if pr.cat_probs is None else [float(x) for x in pr.cat_probs]
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)
    ranges, leafvec = [], {}
    for v in range(n):
        if pb.leaf_taxon[v] >= 0:
            leafvec[v] = MR.leaf_vector(pb, pr, f, v)
            ranges.append([c for c in range(M + 1) if leafvec[v][c] != 0.0])
        elif v == root:
            ranges.append(list(range(1, R + 1)))
        else:
            ranges.append(list(range(M + 1)))
    top = max(M, R)
    post = np.zeros((n, top + 1))
    full = np.zeros((n, 2 * top + 1))
    Z = 0.0
    for k in range(len(mats)):
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
            w *= probs[k] * prior[assign[root] - 1]
            Z += w
            for v in range(n):
                post[v][assign[v]] += w
                if v != root:
                    full[v][assign[v] - assign[pb.parent[v]] + top] += w
    return summarise_family(pb, {"full": full, "post": post, "Z": Z}, D, level)


KEYS = ("pmf", "below", "above", "mean", "mode", "lo", "hi", "mode_gap", "lo_gap", "hi_gap", "node_mean", "mean_scale")


def diagonals(pb, pr, mats, families=None, mutant=None):
    """The pass of all (or the listed) families: a list of diagonals_family's states."""
    fams = range(pb.n_families) if families is None else families
    return [diagonals_family(pb, pr, mats, f, mutant) for f in fams]


def summarise(pb, states, D, level, mutant=None):
    """-> arrays shaped like Context.branch_change's, plus the tie measures, node_mean and mean_scale."""
    rows = [summarise_family(pb, st, D, level, mutant) for st in states]
    out = {k: np.stack([r[k] for r in rows]) for k in KEYS}
    out["log_evidence"] = np.array([r["log_evidence"] for r in rows])
    out["failed"] = np.array([r["failed"] for r in rows], dtype=np.int32)
    return out


def change(pb, pr, mats, D, level, families=None, mutant=None):
    return summarise(pb, diagonals(pb, pr, mats, families, mutant), D, level, mutant)


def max_shift(mut, ref):
    """The largest absolute difference of any probability or mean between two results (NaN patterns must agree)."""
    worst = 0.0
    for key in ("pmf", "below", "above", "mean"):
        g, r = np.asarray(mut[key]), np.asarray(ref[key])
        assert np.array_equal(np.isnan(g), np.isnan(r)), key
        ok = ~np.isnan(r)
        if ok.any():
            worst = max(worst, float(np.max(np.abs(g[ok] - r[ok]))))
    return worst


def compare(got, ref, label):
    """The GPU test's comparison; prints every figure before it asserts.  pmf and tails: 1e-10 relative, an entry whose
    reference value is below 1e-250 absolutely against 1e-250; mean: 1e-10 of max(1, the larger node mean); mode, lo, hi
    exact except where the reference is within 1e-9 of a tie; NaN, CAFE_CHANGE_NONE and failed exactly.  Returns the share
    of integer cells the reference excuses."""
    assert np.array_equal(got["failed"], ref["failed"]), label
    for key in ("pmf", "below", "above", "log_evidence"):
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape, (label, key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key)
        ok = ~np.isnan(r)
        bound = np.where(np.abs(r[ok]) < 1e-250, 1e-250, 1e-10 * np.abs(r[ok]))
        ratio = np.abs(g[ok] - r[ok]) / bound
        worst = float(ratio.max()) if ratio.size else 0.0
        print("%s %s: worst |d| / bound = %.3g" % (label, key, worst))
        assert worst <= 1.0, (label, key, worst)
    g, r = np.asarray(got["mean"]), np.asarray(ref["mean"])
    assert np.array_equal(np.isnan(g), np.isnan(r)), (label, "mean")
    ok = ~np.isnan(r)
    ratio = np.abs(g[ok] - r[ok]) / (1e-10 * np.asarray(ref["mean_scale"])[ok])
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%s mean: worst |d| / bound = %.3g" % (label, worst))
    assert worst <= 1.0, (label, "mean", worst)
    n_exc = n_cells = 0
    for key in ("mode", "lo", "hi"):
        mask = ref[key + "_gap"] <= 1e-9
        diff = np.asarray(got[key]) != np.asarray(ref[key])
        print("%s %s: %d differ, %d excusable of %d" % (label, key, int(diff.sum()), int(mask.sum()), diff.size))
        assert not np.any(diff & ~mask), (label, key, np.argwhere(diff & ~mask)[:5])
        n_exc += int(mask.sum())
        n_cells += diff.size
    return n_exc / n_cells


# ---------------------------------------------------------------------------------------- the tables the tests share
# tests/missing_ref.py's tree (seven taxa: a cherry, a leaf beside it, a polytomy of three leaves, a node with two interior
# children, a leaf under the root) and its table with every cell observed: the all-zero family, 300 distinct families in the
# order of their largest count, then rows that repeat earlier ones; and four families of this file with the whole clade
# ((A,B),G) at zero beside positive counts, where an interior node and its parent are both extinct with material probability
# (the i = 0 row of the joint).  312 families, 305 distinct columns (three 128-column tiles, the last partial), at order 41
# (M 40, R 30) and order 300 (M 299, R 250).
def _tables():
    import missing_ref as MS
    return MS


MODELS = ("base", "gamma", "two_lambdas", "death_rates", "error3", "error5")


CLADE_AT_ZERO = np.array([[0, 0, 1, 2, 1, 0, 1], [0, 0, 3, 2, 2, 0, 2], [0, 0, 0, 1, 0, 0, 1], [0, 0, 2, 4, 3, 0, 0]], dtype=np.int32)     # columns: A B C D E G H


def table(order):
    MS = _tables()
    assert MS.SPECIES == ["A", "B", "C", "D", "E", "G", "H"]
    return np.concatenate([MS.table(order, blank=False), CLADE_AT_ZERO])


def problem(order, model="base"):
    return _tables().problem(order, model, counts=table(order))


def params(pb, model="base"):
    return _tables().params(pb, model)


def death_rates(model):
    return _tables().death_rates(model)


def root_above_problem():
    """Order 41 with R > M: M = 30, R = 40, the order-41 table cut at 30."""
    from cafexp_amd import problem as P
    MS = _tables()
    counts = np.minimum(MS.table(41, blank=False), 30).astype(np.int32)
    pb = P.build_problem(P.parse_newick(MS.NEWICK), MS.SPECIES, ["f%d" % i for i in range(len(counts))], counts, root_filter=False,
                         max_family_size=30, max_root_family_size=40)
    assert pb.matrix_size == 41 and pb.max_family_size == 30 and pb.max_root_family_size == 40
    return pb
