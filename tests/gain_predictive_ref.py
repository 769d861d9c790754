"""Leave-one-out predictive distribution of a leaf count under the gain model, by its definition (a helper, not a test): no down
pass, only the prune of tests/gain_ref.py.  w[y] is the sum-rule evidence of the family with leaf l's count REPLACED by y,
y = 0..M; the distribution is w / sum(w).  With an error model leaf_vector applies the taps of y, so y is the observed value."""
import numpy as np

import gain_ref as G

KEYS = ("mean", "sd", "p_below", "p_obs", "p_above")


def root_vectors(pb, counts, mats, error_model=None):
    """L[taxon][y][0..R]: the root likelihoods of the family with the taxon's count replaced by y"""
    out = []
    for t in range(pb.n_taxa):
        c = np.array(counts, dtype=np.int64)
        out.append([])
        for y in range(pb.max_family_size + 1):
            c[t] = y
            out[-1].append(G.root_likelihoods(pb, c, mats, error_model))
    return np.array(out)


def summary(w, counts):
    """KEYS (and second, E[(y - x)^2], the scale of the variance's error) per taxon from w[taxon][0..M]; x = 0 and NaN p's for a missing cell"""
    y = np.arange(w.shape[1], dtype=np.float64)
    out = {k: np.full(len(counts), np.nan) for k in KEYS + ("second",)}
    for t, x in enumerate(counts):
        p, d = w[t] / w[t].sum(), y - max(int(x), 0)
        m1, out["second"][t] = p @ d, p @ d ** 2
        out["mean"][t], out["sd"][t] = max(int(x), 0) + m1, np.sqrt(max(out["second"][t] - m1 * m1, 0.0))
        if x >= 0:
            out["p_below"][t], out["p_obs"][t], out["p_above"][t] = p[:x].sum(), p[x], p[x + 1:].sum()
    return out


def table(pb, families, rates, prior, root_absent, error_model=None, cache=None):
    """summary() of every listed family (-1: the all-zero profile) under ONE rate set, stacked [n][n_taxa]; cache keeps the
    root vectors, which do not depend on root_absent"""
    cache = {} if cache is None else cache
    mats, rows = None, []
    for f in families:
        counts = np.zeros(pb.n_taxa, dtype=np.int64) if f < 0 else pb.counts[f]
        if int(f) not in cache:
            mats = mats or G.matrices(pb, *rates)
            cache[int(f)] = root_vectors(pb, counts, mats, error_model)
        w = np.exp([[G.reduce_root(L, prior, root_absent, "sum") for L in per_taxon] for per_taxon in cache[int(f)]])
        rows.append(summary(w, counts))
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}
