"""CPU side of tests/test_magnitude_audit.py: likelihood panels by numpy products from any set of matrices, families whose
likelihood lies at the edge of fp64, and the audit of the k-steps that the magnitude rule (extents.hip, "Magnitudes") leaves
out of a K2 op.  Nothing here touches the device: the tests hand in what they read back from it."""
import dataclasses

import numpy as np

TINY = 2.2e-308                  # just below the smallest normal double, 2.2250738585072014e-308
NORMAL_TOP = 1e-250              # upper end of the second band of edge families
SKIP_LOG2 = -1077.0              # four products below 2^-1077 sum to less than 2^-1075, half the smallest denormal
# the two calls of tests/test_magnitude_skip.py, (lambda, gamma model with K = 2 at ALPHA)
CALLS = {"gamma": (0.002, True), "base": (0.0015, False)}
ALPHA = 0.9


def children_of(pb):
    kids = [[] for _ in pb.parent]
    for v, p in enumerate(pb.parent):
        if p >= 0:
            kids[p].append(v)
    return kids


def interior_non_root(pb):
    return [v for v in range(len(pb.parent)) if pb.leaf_taxon[v] < 0 and pb.parent[v] >= 0]


def root_of(pb):
    return int(np.flatnonzero(np.asarray(pb.parent) < 0)[0])


def oracle_matrices(oracle, pb, lambdas, mult=1.0):
    """{node: the oracle's matrix of the branch above it} for one rate category (lambda = mu)."""
    n = pb.matrix_size
    built = {}
    out = {}
    for v in range(len(pb.parent)):
        if pb.parent[v] < 0:
            continue
        key = (float(lambdas[pb.lambda_index[v]] * mult), float(pb.branch_length[v]))
        if key not in built:
            built[key] = oracle.build_matrix(n, key[0], key[1], fast=True)
        out[v] = built[key]
    return out


def cpu_panels(pb, mats, counts):
    """{interior node: its likelihood panel}, one column per row of `counts`, by numpy products from mats[v], the matrix
    P[s][c] of the branch above v.  A non-root panel has the rows s = 0 .. M, the root's the rows s = 1 .. R."""
    M, R = pb.max_family_size, pb.max_root_family_size
    kids = children_of(pb)
    panels = {}
    for v in range(len(pb.parent)):                          # children come before their parents
        if pb.leaf_taxon[v] >= 0:
            continue
        rows = slice(1, R + 1) if pb.parent[v] < 0 else slice(0, M + 1)
        L = None
        for u in kids[v]:
            if pb.leaf_taxon[u] >= 0:
                f = mats[u][rows, counts[:, pb.leaf_taxon[u]]]
            else:
                f = mats[u][rows, :M + 1] @ panels[u]
            L = f if L is None else L * f
        panels[v] = L
    return panels


def edge_rows(oracle, pb, lambdas, mult, per_band=8, productive_tips=1, strict=True):
    """(count rows for families at the edge of fp64 under the rates lambdas * mult, how many of them form the first group):
    copies of family 0 with one tip lowered (where a tip lowered to 1 still leaves the largest root likelihood above 1e-250,
    that tip stays at 1 and the next one is lowered as well).  Per productive tip up to `per_band` rows whose largest root
    likelihood lies in [2.2e-308, 1e-250] -- the first group -- and as many where it is denormal -- the second --, picked
    from the likelihood of every candidate value computed with the ORACLE's matrices and numpy products; the caller asserts
    the bands with oracle.prune.  strict=False: where the rates are so large that no tip gets there, the copies of family 0
    with one, two, ... tips at 1 instead -- the least likely families there are.

    One productive tip by default: a panel bound is a product of per-leaf maxima over a column tile, so families (x, 598) and
    (598, x) at a cherry in one tile are bounded like a family (598, 598) -- by 2^-8 and not by 2^-1000 -- and the K ranges of
    their tile would be those of an ordinary family."""
    mats = oracle_matrices(oracle, pb, lambdas, mult)
    root = root_of(pb)
    base = np.array(pb.counts[0], dtype=np.int32)
    norm_rows, deno_rows, lowered, done = [], [], [], 0
    # the largest tips first, they have the longest way down, but never the first of them: a row keeps family 0's largest count
    # and with it its place in the order of the columns, behind family 0
    for tip in np.argsort(-base, kind="stable")[1:]:
        if done == productive_tips or base[tip] < 3:
            break
        xs = np.arange(1, base[tip], dtype=np.int32)
        cand = np.repeat(base[None, :], len(xs), axis=0)
        cand[:, tip] = xs
        top = cpu_panels(pb, mats, cand)[root].max(axis=0)
        if not top.any():
            break                                            # (too many tips at 1 by now)
        deno = xs[(top > 0) & (top < TINY)]
        # (clear of zero where there is room: the oracle's own summation order may round the last denormals away)
        deno = deno[min(2, max(0, len(deno) - per_band)):]
        norm = xs[(top >= TINY) & (top <= NORMAL_TOP)]
        if len(deno) < 3 or len(norm) < 3:
            base[tip] = 1
            lowered.append(base.copy())
            continue
        for band, dest in ((norm, norm_rows), (deno, deno_rows)):
            for x in band[np.unique(np.linspace(0, len(band) - 1, per_band).astype(np.int64))]:
                row = base.copy()
                row[tip] = x
                dest.append(row)
        done += 1
    if done == 0 and not strict:
        norm_rows, deno_rows = lowered[:len(base) // 2], []
    else:
        assert done >= 1, "no tip of family 0 reaches the edge of fp64"
    rows = norm_rows + deno_rows
    return np.array(rows, dtype=np.int32).reshape(len(rows), len(base)), len(norm_rows)


def with_rows(pb, rows, sort=False):
    """(pb with `rows` appended, indices of the appended families).  sort: families in the stable order of their largest
    count -- the order a context without dedup gives its panel columns, so that column f is family f."""
    counts = np.ascontiguousarray(np.vstack([pb.counts, rows]), dtype=np.int32)
    assert counts.max() <= pb.max_family_size
    idx = np.arange(pb.counts.shape[0], counts.shape[0])
    if sort:
        order = np.argsort(counts.max(axis=1), kind="stable")
        counts = np.ascontiguousarray(counts[order])
        inv = np.empty_like(order)
        inv[order] = np.arange(len(order))
        idx = inv[idx]
    ids = ["fam%06d" % i for i in range(counts.shape[0])]
    return dataclasses.replace(pb, counts=counts, family_ids=ids), idx


def edge_problem(oracle, pb, pr, sort=False, strict=True):
    """(pb with the edge families of the call `pr` appended, their indices, their largest root likelihood per category by
    oracle.prune, how many of them form the first group).  The families are chosen in the category with the smallest rate,
    where a discordant family is least likely: under the larger rates the same families are more likely.  strict: in that
    category every family of the first group lies in [2.2e-308, 1e-250] and every one of the second is denormal, at least 3
    each, and none is exactly zero in any category -- by the oracle alone.

    The two groups stand apart because a context without dedup gives its columns to the families in the stable order of their
    largest count: all edge families hold the table's largest, family 0's, so they come last, in this order.  With
    256 - (first group) families in pb the second group has a column tile to itself.  That matters: a tile's bound is that of
    its largest column, and next to a family 60 decades more likely the K ranges of the tile are that family's."""
    mults = [1.0] if pr.multipliers is None else [float(m) for m in pr.multipliers]
    rows, n_first = edge_rows(oracle, pb, pr.lambdas, min(mults), strict=strict)
    out, idx = with_rows(pb, rows, sort=sort)
    tops = np.array([[oracle.prune(out, pr, int(f), mult=m, fast=True).max() for m in mults] for f in idx]).reshape(len(idx), len(mults))
    if strict:
        low = tops[:, int(np.argmin(mults))]
        assert n_first >= 3 and len(idx) - n_first >= 3 and (tops > 0).all(), tops.tolist()
        assert ((low[:n_first] >= TINY) & (low[:n_first] <= NORMAL_TOP)).all() and (low[n_first:] < TINY).all(), tops.tolist()
    return out, idx, tops, n_first


def band_counts(tops):
    """tops [families][categories]: largest root likelihood.  -> (denormal, low normal, exactly zero) family counts, a family
    counting for a band when it lies there in SOME category and as zero when it is zero in ANY."""
    tops = np.asarray(tops, dtype=np.float64).reshape(len(tops), -1)
    deno = ((tops > 0) & (tops < TINY)).any(axis=1)
    norm = ((tops >= TINY) & (tops <= NORMAL_TOP)).any(axis=1)
    return int(deno.sum()), int(norm.sum()), int((tops == 0).any(axis=1).sum())


def _log2(a):
    with np.errstate(divide="ignore"):
        return np.log2(a)                                    # (denormals included; log2(0) = -inf)


def block_step_max(P, M, n_blocks, n_ksteps):
    """[16-row block b][k-step ks]: the largest P[s][c] over the parent sizes s = 16 b + 1 .. 16 b + 16 and the child sizes
    c = 4 ks .. 4 ks + 3 (c <= M: the contraction ends there)."""
    n = P.shape[0]
    A = np.zeros((16 * n_blocks, 4 * n_ksteps))
    rows, cols = min(n - 1, 16 * n_blocks), min(M + 1, 4 * n_ksteps, P.shape[1])
    A[:rows, :cols] = P[1:1 + rows, :cols]
    return A.reshape(n_blocks, 16, n_ksteps, 4).max(axis=(1, 3))


def tile_step_max(L, n_tiles, n_ksteps):
    """[column tile ct][k-step ks]: the largest L[c][f] over c = 4 ks .. 4 ks + 3 and the columns f of 128-column tile ct."""
    B = np.zeros((4 * n_ksteps, 128 * n_tiles))
    rows = min(L.shape[0], 4 * n_ksteps)
    B[:rows, :L.shape[1]] = L[:rows]
    return B.reshape(n_ksteps, 4, n_tiles, 128).max(axis=(1, 3)).T


def audit_skipped_steps(P, L, M, new, old):
    """The proof obligation of the magnitude rule for one K2 op.  P: the matrix, L: the panel it multiplies (rows 0 .. M, one
    column per family), new / old: k_ranges of the default context and of CAFE_NO_MAGSKIP=1, [tiles][blocks][2].
    -> (k-steps inside old and outside new, how many of them hold a non-zero product, the largest log2 of a product in one
    of them, the (tile, block, k-step) where that is), the product of a (tile, block, k-step) being
    max P[s][c] over the block's s and the step's c  x  max L[c][f] over the step's c and the tile's f."""
    new, old = new.astype(np.int64), old.astype(np.int64)
    assert new.shape == old.shape
    n_tiles, n_blocks = new.shape[:2]
    n_ksteps = (M + 1 + 3) // 4
    assert old[..., 1].max() < n_ksteps and 128 * n_tiles >= L.shape[1]
    ks = np.arange(n_ksteps)
    in_old = (ks >= old[..., 0:1]) & (ks <= old[..., 1:2])   # [tiles][blocks][k-steps]
    in_new = (ks >= new[..., 0:1]) & (ks <= new[..., 1:2])
    assert not (in_new & ~in_old).any()                      # (the ranges only ever shrink)
    skipped = in_old & ~in_new
    prod = _log2(block_step_max(P, M, n_blocks, n_ksteps))[None, :, :] + _log2(tile_step_max(L, n_tiles, n_ksteps))[:, None, :]
    prod = np.where(skipped, prod, -np.inf)
    where = np.unravel_index(int(np.argmax(prod)), prod.shape)
    return int(skipped.sum()), int(np.isfinite(prod).sum()), float(prod[where]), tuple(int(i) for i in where)
