"""Plain numpy statement of the joint (Pupko) reconstruction and of the Viterbi branch sums (a helper, not a test).

joint_reconstruct states gene_family_reconstructor.cpp:13-165 and branch_probabilities states compute_viterbi_sum
(:361-400), both on matrices handed in: mats[v] is the full P[i][j] (i = size of v's parent, j = size of v) of the branch
above node v, None at the root, as marginal_ref.oracle_matrices / context_matrices return per category.

Every value the reconstruction compares is a chain of single fp64 multiplies and max: no addition, so no FMA contraction and
no summation order.  The multiplies are written in the association of csrc/reconstruct.hip (which is the reference's):
  leaf      L[j] = P[j][x], j >= 1; L[0] = 0 (the reference's loop starts at 1)
  interior  L_v[i] = max_j P_v[i][j] * B_v[j], i >= 1; L_v[0] = B_v[0] (row 0 of P is e_0, it is not read from the matrix)
  panel     B_parent = product over the children in ascending node index: the first stores, each later one multiplies the
            stored value, (a * b) * c
  root      first arg max over j = 1..min(M, R) of B[j] * float64(rp[j]), a strict > scan from -1
  backtrack first arg max over j = 0..M of B_v[j] * P_v[i][j], i = the parent's state, a strict > scan from -1
  leaves    carry their counts
so on the same matrices the integer states are equal, ties included.  (All products are finite and >= 0: the strict scan from
-1 is np.argmax, which returns the first maximum.)

Because every leaf has L[0] = 0, B_v[0] = 0 at every interior node: an interior node reconstructs to 0 only where its whole
product row is zero (a saturated branch, a pure-birth matrix, underflow), and its own interior children are then read through
row 0.

mutant=: deliberately WRONG statements, for tests that ask whether their inputs can tell (MUTANTS, VITERBI_MUTANTS).
"""
import numpy as np

import marginal_ref as MR

MUTANTS = ("last_argmax",                    # non-strict >=: the last maximum, at the root and on the way down
           "root_scans_from_zero",           # the root scan starts at j = 0
           "root_range_to_M",                # the root scan ignores R: j = 1..M, the prior continued with its last entry
           "leaf_keeps_row_zero",            # L[0] = P[0][x] at a leaf
           "zero_row_takes_first_scanned",   # the way down scans only the non-zero extent [lo, hi] of the matrix row's block of 16
                                             # parent sizes, from -1: on an all-zero product row with lo > 0 it returns lo, not 0
           "row_zero_read_from_matrix")      # parent size 0 treated like any other: the k-major store has no row 0, index i - 1
                                             # clamped to 0 reads row 1 (in L_v[0] and on the way down)
VITERBI_MUTANTS = ("viterbi_includes_M",     # m = 0..M
                   "viterbi_tie_counts_whole")   # entries equal to P[ps][cs] count whole


def _first_argmax(val, mutant):
    if mutant == "last_argmax":
        return len(val) - 1 - int(np.argmax(val[::-1]))
    return int(np.argmax(val))


def block_extent(P, i, M):
    """[lo, hi] of the non-zero entries of the rows of i's block of 16 parent sizes (16 g + 1 .. 16 g + 16), hi cut at M;
    hi < lo for an all-zero block.  What K1 records per block and backtrack_kernel scans."""
    g = (i - 1) >> 4
    nz = np.nonzero((P[16 * g + 1:16 * g + 17] != 0.0).any(axis=0))[0]
    if len(nz) == 0:
        return 1, 0
    return int(nz[0]), min(M, int(nz[-1]))


def joint_reconstruct(pb, rp, mats, mutant=None):
    """-> (states int32 [F][n_nodes], info).  info: via_row0 [F][n_nodes] (an interior node whose parent's state is 0),
    zero_row [F][n_nodes] (an interior node whose whole product row was zero: it takes the first scanned size),
    root_value [F] (the root's winning B[j] * rp[j])."""
    assert mutant is None or mutant in MUTANTS, mutant
    n, M, R, F = pb.n_nodes, pb.max_family_size, pb.max_root_family_size, pb.n_families
    ch, root = MR.children_of(pb), MR.root_of(pb)
    jmax = min(M, R)
    prior = np.asarray(rp, dtype=np.float32).astype(np.float64)
    assert len(prior) >= jmax + 1
    B = [None] * n                                           # B[v][j][f], interior nodes
    for v in range(n):                                       # children before parents
        if v == root:
            continue
        P = mats[v]
        if pb.leaf_taxon[v] >= 0:
            x = pb.counts[:, pb.leaf_taxon[v]].astype(np.int64)
            L = P[:M + 1][:, x].copy()
            if mutant != "leaf_keeps_row_zero":
                L[0] = 0.0
        else:
            L = np.empty((M + 1, F))
            for f in range(F):
                L[:, f] = (P[:M + 1, :M + 1] * B[v][None, :, f]).max(axis=1)
            L[0] = L[1] if mutant == "row_zero_read_from_matrix" else B[v][0]
        p = int(pb.parent[v])
        B[p] = L if B[p] is None else B[p] * L
    states = np.zeros((F, n), dtype=np.int32)
    info = {"via_row0": np.zeros((F, n), dtype=bool), "zero_row": np.zeros((F, n), dtype=bool), "root_value": np.zeros(F)}
    first = 0 if mutant == "root_scans_from_zero" else 1
    last = jmax
    if mutant == "root_range_to_M":
        last = M
        prior = np.concatenate([prior[:jmax + 1], np.full(M - jmax, prior[jmax])])
    for f in range(F):
        val = B[root][first:last + 1, f] * prior[first:last + 1]
        states[f, root] = first + _first_argmax(val, mutant)
        info["root_value"][f] = val.max()
    e0 = np.zeros(M + 1)
    e0[0] = 1.0
    for v in range(n - 1, -1, -1):                           # parents before children
        if v == root:
            continue
        if pb.leaf_taxon[v] >= 0:
            states[:, v] = pb.counts[:, pb.leaf_taxon[v]]
            continue
        P = mats[v]
        for f in range(F):
            i = int(states[f, pb.parent[v]])
            if i == 0:
                row = P[1, :M + 1] if mutant == "row_zero_read_from_matrix" else e0
            else:
                row = P[i, :M + 1]
            val = B[v][:, f] * row
            info["via_row0"][f, v] = i == 0
            info["zero_row"][f, v] = not val.any()
            if mutant == "zero_row_takes_first_scanned" and i > 0:
                lo, hi = block_extent(P, i, M)
                states[f, v] = lo + int(np.argmax(val[lo:hi + 1])) if hi >= lo else 0
            else:
                states[f, v] = _first_argmax(val, mutant)
    return states, info


def branch_probabilities(pb, sizes, mats, mutant=None):
    """compute_viterbi_sum for every (family, node): NaN at the root and where parent size == child size; else the sequential
    sum over m = 0..M-1 of P[ps][m] where it is < P[ps][cs], half of it where it is equal.  Row 0 is e_0."""
    assert mutant is None or mutant in VITERBI_MUTANTS, mutant
    n, M = pb.n_nodes, pb.max_family_size
    sizes = np.asarray(sizes)
    F = sizes.shape[0]
    out = np.full((F, n), np.nan)
    e0 = np.zeros(M + 1)
    e0[0] = 1.0
    top = M + 1 if mutant == "viterbi_includes_M" else M
    half = 1.0 if mutant == "viterbi_tie_counts_whole" else 0.5
    for v in range(n):
        par = int(pb.parent[v])
        if par < 0:
            continue
        for f in range(F):
            ps, cs = int(sizes[f, par]), int(sizes[f, v])
            if ps == cs:
                continue
            row = e0 if ps == 0 else mats[v][ps, :M + 1]
            calc = row[cs]
            pm = row[:top]
            terms = np.where(pm == calc, pm * half, np.where(pm < calc, pm, 0.0))
            out[f, v] = np.cumsum(terms)[-1] if top > 0 else 0.0     # cumsum adds left to right
    return out
