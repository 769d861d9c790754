"""Plain numpy statement of the scorer on a table with missing cells (a helper, not a test), and the tables the tests share.

The rule (include/cafe_mi355x.h): a leaf whose count is CAFE_COUNT_MISSING contributes the factor EXACTLY 1.0 to every parent
size, in every category, with or without an error model -- the family on the tree without that leaf.  `up` is the up pass of
tests/marginal_ref.py over all families at once with that rule; `variant` makes it deliberately WRONG, for the test that asks
whether the tables can tell:
    "zero"    the missing cell scored as an observed 0 (what atoi makes of "NA");
    "rowsum"  the factor taken as the truncated row sum, sum_{c <= M} P[s][c]: the leaf vector all ones;
    "taps"    the error model applied to the unknown count: the leaf vector sum_x err[x][.] over the counts x = 0..M, cut to
              [0, M] (without an error model that is "rowsum").
mats[k][v]: the N x N matrix of the branch above node v in category k, None at the root (marginal_ref.context_matrices reads
the ones a call built; bd_lm_ref.reference_matrices builds them in numpy).

The tree has seven taxa: a cherry on ONE matrix (A, B: equal branch lengths, one lambda class), a leaf whose sibling is interior
(G beside the cherry), a polytomy of three leaves (C, D, E), a node with two interior children and no leaf, and a leaf under the
root (H).  table(order) returns the counts: family 0 has every cell missing; then 300 distinct families in the order of their
largest count, which D always holds and which is never blanked -- so the column of family f in the root's panel (and, without
subtree sharing, in every panel) is f itself (root_columns states the library's rule and the tests assert it); then rows that
repeat earlier ones, and rows that differ from an earlier one by their missing pattern only.
"""
import dataclasses

import numpy as np

import leaf_predictive_ref as LR
import marginal_ref as MR
from cafexp_amd import problem as P
from cafexp_amd.gamma_rates import discrete_gamma

MISSING = P.COUNT_MISSING
NEWICK = "((((A:3,B:3):2,G:5):2,(C:2,D:2.5,E:3):4):3,H:9);"
LAMBDA_TREE = "((((A:1,B:1):1,G:1):1,(C:2,D:2,E:2):2):1,H:2);"
SPECIES = ["A", "B", "C", "D", "E", "G", "H"]
SHAPES = {41: (40, 30, 36), 300: (299, 250, 280)}        # order: M, R, largest count
LAMBDA1 = np.array([0.012])
LAMBDAS = np.array([0.012, 0.006])
MUS = np.array([0.007, 0.009])
N_DISTINCT = 300
MODELS = ("base", "gamma", "two_lambdas", "death_rates", "error3", "error5")

# where the cells are blanked, by family index (= column, see the module text).  Columns 0 / 127 | 128 / 255 | 256 are the first
# and last of the 128-column tiles; 10 is the even column of the pair (10, 11), 13 the odd one of (12, 13), 20 and 21 a whole pair.
TILE_EDGES = (127, 128, 255, 256)
BLANKS = {
    "H": TILE_EDGES + (10, 13, 20, 21),                    # the leaf under the root
    "G": TILE_EDGES + (10, 13, 20, 21) + tuple(range(110, 126, 2)),      # the leaf whose sibling is interior
    "B": tuple(range(30, 61, 3)) + tuple(range(32, 63, 6)),             # one leaf of the cherry ...
    "A": tuple(range(32, 63, 6)) + (34, 40),                            # ... both of them (32, 38, ...), the other one alone
    "C": tuple(range(70, 101, 5)) + tuple(range(71, 102, 10)),          # the polytomy: one leaf, and (71, 81, ...) two
    "E": tuple(range(71, 102, 10)),
}
SOURCE_OF_PATTERN_TWINS = (300, 300)                     # this row comes again with G blanked, and with G and H blanked (the
                                                         # largest family: its twins' columns follow every other)
SOURCE_OF_DUPLICATES = (0, 5, 30, 127, 299)              # these rows come again as they are


def table(order, blank=True):
    """counts [n_families][7] (columns as SPECIES); blank=False: the same families with every cell observed (family 0, which has
    no observed cell at all, becomes all zero -- only the tests that compare the two tables row by row use it)"""
    M, R, cap = SHAPES[order]
    rng = np.random.default_rng(1000 + order)
    d = 1 + (np.arange(N_DISTINCT) * cap) // N_DISTINCT   # the largest count, non-decreasing
    col = {s: j for j, s in enumerate(SPECIES)}
    fixed = np.zeros((N_DISTINCT + 1, len(SPECIES)), dtype=bool)     # the cells blanked by plan
    fixed[0, :] = True
    for s, fams in BLANKS.items():
        fixed[list(fams), col[s]] = True
    rows, seen = [[0] * len(SPECIES)], set()
    for i in range(N_DISTINCT):
        while True:                                       # distinct also after the planned blanks
            row = [int(d[i]) if s == "D" else int(rng.integers(max(0, d[i] - max(2, d[i] // 4)), d[i] + 1)) for s in SPECIES]
            key = tuple(MISSING if b else x for x, b in zip(row, fixed[i + 1]))
            if key not in seen:
                seen.add(key)
                rows.append(row)
                break
    full = np.array(rows, dtype=np.int32)
    counts = np.where(fixed, MISSING, full).astype(np.int32)
    extra = rng.random(counts.shape) < 0.03               # and 3 % of the other cells of the later families, never D
    extra[:150] = False
    extra[list(SOURCE_OF_PATTERN_TWINS)] = False
    extra[:, col["D"]] = False
    counts[extra] = MISSING
    seen = set()
    for i in range(len(counts)):                          # (two families may differ only where one was blanked: that one keeps its cells)
        if tuple(counts[i]) in seen:
            counts[i, extra[i]] = full[i, extra[i]]
        assert tuple(counts[i]) not in seen, i
        seen.add(tuple(counts[i]))
    twins = counts[list(SOURCE_OF_PATTERN_TWINS)].copy()
    twins[:, col["G"]] = MISSING
    twins[1, col["H"]] = MISSING
    counts = np.concatenate([counts, twins, counts[list(SOURCE_OF_DUPLICATES)]])
    full = np.concatenate([full, full[list(SOURCE_OF_PATTERN_TWINS)], full[list(SOURCE_OF_DUPLICATES)]])
    return counts if blank else full


def problem(order, model="base", counts=None, newick=NEWICK, lambda_tree=LAMBDA_TREE, species=SPECIES):
    M, R, _ = SHAPES[order]
    counts = table(order) if counts is None else counts
    two = model in ("two_lambdas", "death_rates")
    pb = P.build_problem(P.parse_newick(newick), species, ["f%d" % i for i in range(len(counts))], counts,
                         lambda_tree=P.parse_newick(lambda_tree, lambda_tree=True) if two else None, root_filter=False,
                         max_family_size=M, max_root_family_size=R, n_deviations={"error3": 3, "error5": 5}.get(model, 0),
                         missing_tokens=("NA",))
    assert pb.matrix_size == order and pb.missing_counts == bool((counts == MISSING).any())
    return pb


def error_model(M, taps):
    row = {3: [0.05, 0.9, 0.05], 5: [0.02, 0.05, 0.86, 0.05, 0.02]}[taps]
    em = np.tile(np.array(row), (M + 1, 1))
    em[0] = {3: [0.0, 0.95, 0.05], 5: [0.0, 0.0, 0.9, 0.06, 0.04]}[taps]
    if taps == 5:
        em[1] = [0.0, 0.05, 0.88, 0.05, 0.02]
    return em


def params(pb, model):
    two = model in ("two_lambdas", "death_rates")
    pr = P.Params(lambdas=(LAMBDAS if two else LAMBDA1).copy(), prior=P.prior_uniform(pb.max_root_family_size))
    if model == "gamma":
        pr.cat_probs, pr.multipliers = discrete_gamma(3, 0.7)
    if model in ("error3", "error5"):
        pr.error_model = error_model(pb.max_family_size, int(model[-1]))
    return pr


def death_rates(model):
    return MUS.copy() if model == "death_rates" else None


def root_columns(counts):
    """The library's column of every family in the root's panel: one per distinct row, in the order of the rows' largest count
    (a missing cell is -1), ties in table order (cafe_create: the sort key at max_element)."""
    first, col_of_row = {}, []
    for row in map(tuple, counts.tolist()):
        col_of_row.append(first.setdefault(row, len(first)))
    reps = sorted(first, key=lambda r: (max(r), first[r]))
    rank = {first[r]: i for i, r in enumerate(reps)}
    return np.array([rank[c] for c in col_of_row])


# ------------------------------------------------------------------------------------------------------------ the prune
def leaf_block(pb, pr, v, variant=None):
    """(B [M+1][F], missing [F]): the leaf vectors of node v, a missing cell's column as the variant says (None: unused)"""
    M, F = pb.max_family_size, pb.n_families
    x = pb.counts[:, pb.leaf_taxon[v]].astype(np.int64)
    miss = x < 0
    xs = np.where(miss, 0, x)
    fam = np.arange(F)
    B = np.zeros((M + 1, F))
    em = pr.error_model
    if em is None:
        B[xs, fam] = 1.0
    else:
        nd = em.shape[1]
        for t in range(nd):
            c = xs - (nd - 1) // 2 + t
            ok = (c >= 0) & (c <= M)
            B[c[ok], fam[ok]] = em[xs[ok], t]
    if variant == "rowsum" or (variant == "taps" and em is None):
        B[:, miss] = 1.0
    elif variant == "taps":
        e = np.zeros(M + 1)
        nd = em.shape[1]
        for y in range(M + 1):
            for t in range(nd):
                c = y - (nd - 1) // 2 + t
                if 0 <= c <= M:
                    e[c] += em[y, t]
        B[:, miss] = e[:, None]
    return B, miss


def up(pb, pr, P_k, variant=None):
    """B, F per node ([rows][F] arrays) of one category: marginal_ref's up pass, a missing leaf's factor exactly 1"""
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    ch, root = MR.children_of(pb), MR.root_of(pb)
    B, Fac = [None] * n, [None] * n
    for v in range(n):
        if pb.leaf_taxon[v] >= 0:
            continue
        top = R if v == root else M
        b = np.ones((top + 1, pb.n_families))
        for c in ch[v]:
            if pb.leaf_taxon[c] >= 0:
                Bc, miss = leaf_block(pb, pr, c, variant)
                Fac[c] = P_k[c][:top + 1, :M + 1] @ Bc
                if variant is None:
                    Fac[c][:, miss] = 1.0
            else:
                Fac[c] = P_k[c][:top + 1, :M + 1] @ B[c]
            b = b * Fac[c]
        B[v] = b
    return B, Fac


def family_lnl(pb, pr, mats, variant=None, root_rule="max"):
    """What cafe_score returns per family (cafe_family_out::family_lnl) under either root rule"""
    R, root = pb.max_root_family_size, MR.root_of(pb)
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)[:R, None]
    inside = [up(pb, pr, mats[k], variant)[0][root][1:R + 1] for k in range(len(mats))]
    with np.errstate(divide="ignore"):
        if pr.multipliers is None:
            t = np.log(inside[0]) + np.log(prior)
            m = t.max(axis=0)
            return m if root_rule == "max" else m + np.log(np.exp(t - m[None, :]).sum(axis=0))
        lik = sum(p * ((L * prior).max(axis=0) if root_rule == "max" else (L * prior).sum(axis=0)) for p, L in zip(pr.cat_probs, inside))
        return np.log(lik)


def predictive(pb, pr, mats):
    """cafe_leaf_predictive on a table with missing cells: leaf_predictive_ref.reference's outputs (updown route), a missing
    leaf's factor 1 in every message; for a missing cell mean and sd are the prediction and the three tails NaN."""
    n, M, R, F = pb.n_nodes, pb.max_family_size, pb.max_root_family_size, pb.n_families
    ch, root = MR.children_of(pb), MR.root_of(pb)
    probs = [1.0] if pr.cat_probs is None else [float(p) for p in pr.cat_probs]
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)[:R]
    u = {v: np.zeros((M + 1, F)) for v in range(n) if pb.leaf_taxon[v] >= 0}
    Z = np.zeros(F)
    for k, pk in enumerate(probs):
        B, Fac = up(pb, pr, mats[k])
        O = [None] * n
        O[root] = np.zeros((R + 1, F))
        O[root][1:] = prior[:, None]
        Z += pk * (O[root] * B[root]).sum(axis=0)
        for p in range(n - 1, -1, -1):
            if pb.leaf_taxon[p] >= 0:
                continue
            top = R if p == root else M
            for v in ch[p]:
                G = O[p].copy()
                for s in ch[p]:
                    if s != v:
                        G = G * Fac[s]
                Ov = mats[k][v][:top + 1, :M + 1].T @ G
                if pb.leaf_taxon[v] >= 0:
                    u[v] += pk * Ov
                else:
                    O[v] = Ov
    out = {key: np.full((F, pb.counts.shape[1]), np.nan) for key in LR.KEYS}
    y = np.arange(M + 1)[:, None]
    fam = np.arange(F)
    for v, uv in u.items():
        w = LR._observe(pr, M, uv)
        t = int(pb.leaf_taxon[v])
        x = pb.counts[:, t].astype(np.int64)
        miss = x < 0
        W = w.sum(axis=0)
        d = y - np.where(miss, 0, x)[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = (y * w).sum(axis=0) / W
            var = ((y - mean[None, :]) ** 2 * w).sum(axis=0) / W
            cols = {"mean": mean, "sd": np.sqrt(var), "p_obs": np.where(miss, np.nan, w[np.where(miss, 0, x), fam] / W),
                    "p_above": np.where(miss, np.nan, np.where(d > 0, w, 0.0).sum(axis=0) / W),
                    "p_below": np.where(miss, np.nan, np.where(d < 0, w, 0.0).sum(axis=0) / W)}
        bad = ~((W > 0) & np.isfinite(W))
        for key, val in cols.items():
            out[key][:, t] = np.where(bad, np.nan, val)
    failed = ~((Z > 0) & np.isfinite(Z))
    out["failed"] = failed.astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["log_evidence"] = np.where(failed, np.nan, np.log(Z))
    return out


def rel(got, want, near_zero=()):
    """largest |got - want| / |want| over the entries, infinities and NaN matched exactly.

    near_zero: the indices of the families with EVERY cell missing, and of those only.  Such a family has lnL = log(1 - 2e-6)
    under the sum rule: the terms of its log-sum-exp are +-3.4 (log of the uniform prior over 30 sizes), so the doubles of the
    REFERENCE hold it to 3.4 eps = 7.5e-16, which is 3.8e-10 of the value -- a relative bound on a logarithm near zero asks more
    than either side can hold.  For these entries the denominator is max(|want|, 1): the bound is 1e-10 on the likelihood itself
    (|d lnL| = |dL| / L) while |lnL| < 1.  Every other entry is held to the plain relative difference."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (got[~fin], want[~fin])
    den = np.abs(want)
    for i in near_zero:
        den[i] = max(den[i], 1.0)
    return float((np.abs(got[fin] - want[fin]) / den[fin]).max(initial=0.0))


def all_missing(pb):
    """indices of the families of pb with every cell missing (rel's near_zero)"""
    return np.where((pb.counts < 0).all(axis=1))[0].tolist()


def with_flag(pb, on=True):
    return dataclasses.replace(pb, missing_counts=on)
