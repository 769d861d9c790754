"""The prune of tests/gain_ref.py and the down pass of tests/gain_posterior_ref.py in np.longdouble on the fp64 matrices (a
helper, not a test): the reference of the scaled dense gain path, whose families' likelihoods lie below fp64's range."""
import numpy as np

import gain_posterior_ref as GP
import gain_ref as G
import marginal_ref as MR

LD = np.longdouble
WIDE = np.finfo(LD).minexp <= -16000           # an extended exponent range: without it this is no reference


def table(pb, families, rates, prior, root_absent):
    """GP.down_pass's dict of every listed family (an index, or -1 for the all-zero profile) under ONE rate set (lambda, mu, nu),
    stacked as float64, with lnl_max (the max rule's value) and top (the largest root likelihood, in longdouble) beside it"""
    M, Rr, nn, ch, root = pb.max_family_size, pb.max_root_family_size, pb.n_nodes, MR.children_of(pb), MR.root_of(pb)
    mats = [None if m is None else m.astype(LD) for m in G.matrices(pb, *[[r] for r in rates])]
    order, rows = [root], []
    for v in order:                                # (grows while it is walked: parents in front of their children)
        order.extend(ch[v])
    for counts in [np.zeros(pb.n_taxa, dtype=np.int64) if f < 0 else pb.counts[f] for f in families]:
        L, factor, outside = {}, {}, {root: GP.root_mass(prior, root_absent, Rr).astype(LD)}
        for v in reversed(order):                  # a factor has the sizes of its parent: R + 1 under the root, M + 1 below
            L[v] = np.prod([factor[u] for u in ch[v]], axis=0) if ch[v] else G.leaf_vector(pb, None, counts, v).astype(LD)
            if v != root:
                factor[v] = mats[v][:(Rr if pb.parent[v] == root else M) + 1, :M + 1] @ L[v]
        at_root = outside[root] * L[root]
        Z = np.sum(at_root)
        out = {"lnl": np.log(Z), "lnl_max": np.log(np.max(at_root)), "top": np.max(L[root]), "p_gain": np.full(nn, np.nan, dtype=LD),
               "p_loss": np.full(nn, np.nan, dtype=LD), "posterior": np.zeros((nn, pb.matrix_size), dtype=LD)}
        for u in order[1:]:
            w = np.prod([outside[int(pb.parent[u])]] + [factor[v] for v in ch[int(pb.parent[u])] if v != u], axis=0)
            outside[u] = w @ mats[u][:len(w), :M + 1]
            out["p_gain"][u] = w[0] * (mats[u][0, 1:M + 1] @ L[u][1:]) / Z
            out["p_loss"][u] = L[u][0] * (w[1:] @ mats[u][1:len(w), 0]) / Z
        for u in order:
            out["posterior"][u, :len(L[u])] = outside[u] * L[u] / Z
        out["p_absent"], out["mean"] = out["posterior"][:, 0], out["posterior"] @ np.arange(pb.matrix_size)
        rows.append(out)
    return {k: np.array([r[k] for r in rows], dtype=LD if k == "top" else np.float64) for k in rows[0]}
