"""Plain np.longdouble statement of cafe_gain_marginal_dense (a helper, not a test): the up and down passes of
tests/gain_posterior_ref.py on the fp64 matrices of tests/gain_ref.py, then per node mean / first arg max / equal-tailed interval of
posterior_u = outside_u L_u / Z, and per branch the joint J[s][c] = w[s] P[s][c] L_u[c] / Z summed over c > s (p_increase), c < s
(p_decrease) and c = s (p_same).  The CDF is the running sum of the posterior as it is (total 1, not renormalised); a threshold it
never reaches gives the node's last size.  A leaf without an error model is its observed count.  `wrong` gets the split wrong on
purpose; cdf_gap and top_gap are the margins the GPU test's integer comparisons rest on (tests/test_gain_marginal_model.py)."""
import numpy as np

import gain_posterior_ref as GP
import gain_ref as G
import marginal_ref as MR

LD = np.longdouble
WRONG, DOUBLES, INTS = ("swapped", "diagonal_in_increase", "diagonal_left_out"), ("mean", "p_increase", "p_decrease", "p_same"), ("mode", "lo", "hi")


def family(pb, counts, mats, prior, root_absent, level, error_model=None, wrong=None):
    """{lnl, the seven outputs [n_nodes], cdf_gap, top_gap: the two margins} of one family; mats in longdouble"""
    M, Rr, nn, ch, root = pb.max_family_size, pb.max_root_family_size, pb.n_nodes, MR.children_of(pb), MR.root_of(pb)
    order = [root]
    for v in order:                                # (grows while it is walked: parents in front of their children)
        order.extend(ch[v])
    L, factor, outside = {}, {}, {root: GP.root_mass(prior, root_absent, Rr).astype(LD)}
    for v in reversed(order):
        L[v] = np.prod([factor[u] for u in ch[v]], axis=0) if ch[v] else G.leaf_vector(pb, error_model, counts, v).astype(LD)
        if v != root:
            factor[v] = mats[v][:(Rr if pb.parent[v] == root else M) + 1, :M + 1] @ L[v]
    Z = np.sum(outside[root] * L[root])
    out = {k: np.full(nn, np.nan, dtype=LD) for k in DOUBLES}
    out.update({k: np.full(nn, -1, dtype=np.int32) for k in INTS}, lnl=np.log(Z), cdf_gap=LD(1), top_gap=LD(1))
    tlo, thi = (1 - LD(level)) / 2, 1 - (1 - LD(level)) / 2
    for u in order:
        if u != root:
            w = np.prod([outside[int(pb.parent[u])]] + [factor[v] for v in ch[int(pb.parent[u])] if v != u], axis=0)
            Pm = mats[u][:len(w), :M + 1]
            outside[u] = w @ Pm
            J = w[:, None] * Pm * L[u][None, :] / Z
            up, down, same = np.triu(J, 1).sum(), np.tril(J, -1).sum(), np.trace(J)
            out["p_increase"][u], out["p_decrease"][u], out["p_same"][u] = {"swapped": (down, up, same), "diagonal_in_increase": (up + same, down, same),
                                                                            "diagonal_left_out": (up, down, LD(0))}.get(wrong, (up, down, same))
        post = outside[u] * L[u] / Z
        out["mean"][u] = np.arange(len(post)) @ post
        x = int(counts[pb.leaf_taxon[u]]) if not ch[u] else -1
        if x >= 0 and error_model is None:
            out["mode"][u] = out["lo"][u] = out["hi"][u] = x
            continue
        live = np.arange(len(post)) if ch[u] else np.nonzero(L[u])[0]      # a leaf's CDF runs over its taps
        cdf = np.cumsum(post[live])
        out["mode"][u] = live[np.argmax(post[live])]
        for key, t in (("lo", tlo), ("hi", thi)):
            hit = np.nonzero(cdf >= t)[0]
            out[key][u] = live[hit[0]] if len(hit) else live[-1]
        top = np.sort(post[live])[::-1]
        out["cdf_gap"] = min(out["cdf_gap"], np.min(np.abs(cdf - tlo)), np.min(np.abs(cdf - thi)))
        if len(top) > 1 and top[1] > 0:
            out["top_gap"] = min(out["top_gap"], (top[0] - top[1]) / top[0])
    return out


def table(pb, families, rates, prior, root_absent, level, error_model=None, wrong=None):
    """family() of every listed family (an index, or -1 for the all-zero profile) under ONE rate set (lambda, mu, nu), stacked"""
    mats = [None if m is None else m.astype(LD) for m in G.matrices(pb, *[[r] for r in rates])]
    rows = [family(pb, np.zeros(pb.n_taxa, dtype=np.int64) if f < 0 else pb.counts[f], mats, prior, root_absent, level, error_model, wrong)
            for f in families]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


# What tests/test_gain_marginal_gpu.py runs.  Short and long branches side by side (p_same > 0.3 on the short ones), lambda != mu.
TREES = {"cherry": "(A:4.5,B:31);", "caterpillar": "((((A:3,B:28):17,C:9):2.5,D:44):12,E:6);", "three": "((A:5,B:19,C:40):14,D:2,(E:8,F:33):27);",
         "balanced": "(((A:3,B:21):9,(C:30,D:5):16):7,((E:12,F:2.5):25,(G:18,H:40):4):11);"}
RATES, ABSENT, LEVEL = (0.0051, 0.00408, 0.00102), 0.2, 0.9
# (M, R, tree, error model): M + 1 = 63 one row tile; 64 exactly one; 65 a second row tile of one row, under a root of fewer
# (R + 1 = 41: its children contract over less than a row tile) and of more sizes (91); 80 a K tile that ends inside the straddling
# range; 129 three row tiles
CASES = [(62, 62, "caterpillar", False), (62, 70, "cherry", True), (63, 63, "balanced", True), (64, 40, "three", False), (64, 90, "three", False),
         (64, 64, "caterpillar", True), (79, 79, "three", False), (128, 128, "balanced", False)]


def problem(M, Rr, tree, error):
    """(problem, params): four families -- about M / 2 with a spread, patchy small counts, ones with two larger, near M (one at M)"""
    from cafexp_amd import problem as P
    from helpers import _explicit_problem
    names = sorted(c for c in TREES[tree] if c.isalpha())
    spread, top = [-5, 4, 0, 7, -3, 2, -6, 5], [0, 9, 5, 12, 7, 3, 10, 6]
    rows = [[M // 2 + d for d in spread], [0, 1, 1, 2, 0, 0, 3, 1], [1, 1, 6, 1, 2, 1, 1, 4], [M - d for d in top]]
    pb = _explicit_problem(TREES[tree], [dict(zip(names, r)) for r in rows], M, Rr)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(Rr))
    if error:
        pb.n_deviations = 3
        pr.error_model = np.tile(np.array([0.07, 0.8, 0.13]), (M + 1, 1))
        pr.error_model[0] = [0.0, 0.9, 0.1]
    return pb, pr
