"""cafe_pvalues (csrc/pvalues.hip) restated in numpy, CPU only: the simulation draw for draw, the sort and the p-value rule.

The generator, the uniform and the inverse-CDF draw are tests/test_simulate_replay.py's (tree_sampler.h restated); what is
restated here is pvalues.hip's own simulate_kernel:
  family f = s * n_sim + i has root size s (s = 0 .. R - 1, i = 0 .. n_sim - 1);
  nodes run from the highest index down (parents have larger indices: parents first);
  the draw of (family f, node v) is uniform01(f, v, 0, seed) into row `parent size` of np.cumsum(mat[:, :M], axis=1), mat the
  order-N matrix of the branch above v, N = max(M, R) + 1 -- sizes 0 .. M - 1 carry the weights;
  no draw is made below an extinct parent (size 0 stays 0).
A draw within AMBIGUOUS = 2^-40 of a CDF entry (of the row total) marks its family ambiguous: the device sums a row by a 64-lane
scan plus carry, numpy sequentially (test_simulate_replay's rule and bound).  The matrix source is passed in.

P-values twice: pvalues() is the plain rule -- np.sort, np.searchsorted(side="right"), an index n reported as n - 1, the maximum
over root sizes, divided by n (probability.cpp:379-407).  pvalue_interval() is what that rule can give when the observed value
and the simulated values are each only known to REL = 1e-10: p_lo counts the entries below v (1 - REL), p_hi those up to
v (1 + REL).  1e-10 is what test_driver_pvalues_match_compiled_reference grants the conditional distributions, ten times the
1e-11 at which cafe_root_max is held to the oracle (two such errors, 2e-11, lie well inside it)."""
import dataclasses

import numpy as np

from test_simulate_replay import AMBIGUOUS, LEFT_OUT, draw, uniform01

assert AMBIGUOUS == 2.0 ** -40 and LEFT_OUT == 1e-4
REL = 1e-10


def oracle_matrices(oracle):
    """matrices(N, lambdas, mus, ts) over oracle.build_matrix (lambda = mu only; it applies the key quantization itself)."""
    def matrices(N, lams, mus, ts):
        assert mus is None
        cache = {}
        for l, t in zip(lams, ts):
            if (l, t) not in cache:
                cache[(l, t)] = oracle.build_matrix(N, float(l), float(t), fast=True)
        return np.stack([cache[(l, t)] for l, t in zip(lams, ts)])
    return matrices


def device_matrices(capi):
    """matrices(N, lambdas, mus, ts) over capi.build_matrices (mus None) / capi.build_matrices_lm."""
    def matrices(N, lams, mus, ts):
        return capi.build_matrices(N, lams, ts) if mus is None else capi.build_matrices_lm(N, lams, mus, ts)
    return matrices


def replay(pb, lambdas, n_sim, seed, matrices, mus=None):
    """simulate_kernel on the host.  pb: a problem.Problem (tree, M, R, lambda_index).  mus: the context's death rates, one per
    lambda index, or None.  Returns (sizes [n_nodes][R * n_sim], counts [n_taxa][R * n_sim], ambiguous [R * n_sim])."""
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    N = max(M, R) + 1
    Fs = R * n_sim
    fam = np.arange(Fs)
    root = int(np.where(pb.parent < 0)[0][0])
    branches = [v for v in range(n) if v != root]
    idx = pb.lambda_index[branches]
    lam = np.atleast_1d(np.asarray(lambdas, dtype=np.float64))[idx]
    mu = None if mus is None else np.atleast_1d(np.asarray(mus, dtype=np.float64))[idx]
    mats = matrices(N, lam, mu, pb.branch_length[branches])
    assert mats.shape == (len(branches), N, N)
    cdf = np.cumsum(mats[:, :, :M], axis=2)
    sizes = np.zeros((n, Fs), dtype=np.int64)
    sizes[root] = fam // n_sim
    ambiguous = np.zeros(Fs, dtype=bool)
    for v in sorted(branches, reverse=True):                 # parents have larger indices: parents first
        ps = sizes[pb.parent[v]]
        size, near = draw(cdf[branches.index(v)][ps], uniform01(fam, v, 0, seed))
        size[ps == 0] = 0                                    # an extinct lineage stays extinct, no draw
        ambiguous |= near & (ps > 0)
        sizes[v] = size
    leaves = np.where(pb.leaf_taxon >= 0)[0]
    return sizes, sizes[leaves[np.argsort(pb.leaf_taxon[leaves])]], ambiguous


def distinct_profiles(pb, counts):
    """(a Problem over the distinct columns of counts [n_taxa][F], the index of every column's profile in it)"""
    uniq, inverse = np.unique(np.ascontiguousarray(counts.T), axis=0, return_inverse=True)
    sub = dataclasses.replace(pb, counts=np.ascontiguousarray(uniq, dtype=np.int32), family_ids=["u%d" % i for i in range(len(uniq))])
    return sub, np.asarray(inverse).reshape(-1)


def prune_root_max(pb, mats):
    """max_j L_root[j], j = 1 .. R, of every family of pb by a plain numpy prune; mats[v]: the order-N matrix of the branch above
    node v (the root's entry is not read).  The reference where the oracle has no model (death rates)."""
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    root = int(np.where(pb.parent < 0)[0][0])
    F = pb.counts.shape[0]
    B = [None] * n
    for v in range(n):                                       # children before parents
        if pb.leaf_taxon[v] >= 0:
            B[v] = np.zeros((M + 1, F))
            B[v][pb.counts[:, pb.leaf_taxon[v]], np.arange(F)] = 1.0
            continue
        top = R if v == root else M
        b = np.ones((top + 1, F))
        for c in np.where(pb.parent == v)[0]:
            b = b * (mats[c][:top + 1, :M + 1] @ B[c])
        B[v] = b
    return B[root][1:R + 1].max(axis=0)


def _positions(cond_sorted, values, side):
    n = cond_sorted.shape[1]
    idx = np.stack([np.searchsorted(row, values, side=side) for row in cond_sorted])     # [R][F]
    idx[idx == n] = n - 1                                    # past the end: index n - 1 (probability.cpp:381)
    return idx.max(axis=0) / n


def pvalues(observed, cond):
    """cond [R][n], sorted or not.  Per observed value: max over rows of the upper-bound position (n -> n - 1) over n."""
    return _positions(np.sort(np.asarray(cond, dtype=np.float64), axis=1), np.asarray(observed, dtype=np.float64), "right")


def pvalue_interval(observed, cond, rel=REL):
    """(p_lo, p_hi): the same rule with every comparison decided against, then for, the simulated values within rel."""
    c = np.sort(np.asarray(cond, dtype=np.float64), axis=1)
    v = np.asarray(observed, dtype=np.float64)
    return _positions(c, v * (1 - rel), "left"), _positions(c, v * (1 + rel), "right")
