"""Plain numpy statements of the leave-one-out predictive distribution of every leaf count (a helper, not a test): what
cafe_leaf_predictive computes.

The model is marginal_ref's: leaf vectors one-hot at the observed count (or the error model's taps), interior sizes 0..M, root
sizes 1..R weighted by the float prior, categories mixed with cat_probs.  mats[k][v] is the N x N matrix (P[parent size][child
size]) of the branch above node v in category k, None at the root: `matrices` builds them in numpy from the quantized keys
(gradient_ref), marginal_ref.context_matrices reads back the ones a call built.  For family f, leaf l with parent p:
    G_l^k[i] = O_p^k[i] prod_{siblings w of l} F_w^k[i]         O_l^k[c] = sum_i P_l^k[i][c] G_l^k[i], c = 0..M
    u = sum_k p_k O_l^k        w[y] = u[y], or with an error model sum_t err[y][t] u[y - half + t], taps outside [0, M] dropped
    W = sum_y w[y]             w[x_l] = Z_f, and nothing else in w depends on x_l
Two routes to w:
  updown   the statement above (what csrc/predictive.hip implements); `mutant` makes it deliberately WRONG (MUTANTS);
  brute    replace x_l by every y in 0..M, take Z(y) from a plain prune (up pass and root sum only): w[y] = Z(y).
Outputs per cell, x the observed count: mean = sum y w / W; var = sum (y - mean)^2 w / W, the central moment taken in a second
pass -- equal to S2 / W - (S1 / W)^2 of the moments about x (or about any point) and free of their cancellation, which at a point
mass away from x leaves sqrt(eps) |x - mean| where the sd is 0; p_below = sum_{y < x} w / W, p_obs = w[x] / W,
p_above = sum_{y > x} w / W.  W zero or not finite: NaN in all five.  log_evidence and failed as marginal_ref's, judged on Z.
"""
import numpy as np

import gradient_ref as GR
import marginal_ref as MR

MUTANTS = ("own_factor_left_in", "err_indexed_at_c", "row0_dropped", "below_includes_x", "mixed_after_normalising")
KEYS = ("mean", "sd", "p_below", "p_obs", "p_above")


def matrices(pb, pr, mus=None):
    """mats[k][v] in numpy from the keys the library quantizes to (rows convolved with the single-lineage law)"""
    out = []
    for k in range(len(GR._mults(pr))):
        cache, row = {}, []
        for key in GR.branch_keys(pb, pr, mus, k):
            if key is not None and key not in cache:
                a, b = GR.alpha_beta(*key)
                cache[key] = GR.matrix(pb.matrix_size, a, b, GR.is_zero(a, b)).real
            row.append(None if key is None else cache[key])
        out.append(row)
    return out


def count_vector(pr, M, y):
    """marginal_ref.leaf_vector for the count y"""
    e = np.zeros(M + 1)
    if pr.error_model is None:
        e[y] = 1.0
        return e
    nd = pr.error_model.shape[1]
    for t in range(nd):
        c = y - (nd - 1) // 2 + t
        if 0 <= c <= M:
            e[c] = pr.error_model[y, t]
    return e


def _observe(pr, M, u, at_c=False):
    """w [M+1][F] from u [M+1][F]; at_c: the error model read at the tap's row (WRONG)"""
    if pr.error_model is None:
        return u.copy()
    nd = pr.error_model.shape[1]
    w = np.zeros_like(u)
    for y in range(M + 1):
        for t in range(nd):
            c = y - (nd - 1) // 2 + t
            if 0 <= c <= M:
                w[y] += pr.error_model[c if at_c else y, t] * u[c]
    return w


def _prune(pb, pr, mats, leafv):
    """Z [F] of the leaf vectors: the up pass and the root sum of every category"""
    root = MR.root_of(pb)
    Z = np.zeros(pb.n_families)
    for k, pk in enumerate(GR._probs(pr)):
        B, _ = GR._up(pb, mats[k], leafv, float)
        O, _ = GR._root_weight(pb, pr, B[root], "sum", False)
        Z += pk * (O * B[root]).sum(axis=0)
    return Z


def _weights_updown(pb, pr, mats, leafv, mutant):
    """w[v] [M+1][F] per leaf v (None elsewhere) and Z [F]"""
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    ch, root = MR.children_of(pb), MR.root_of(pb)
    probs = GR._probs(pr)
    u = [np.zeros((M + 1, pb.n_families)) if pb.leaf_taxon[v] >= 0 else None for v in range(n)]
    Z = np.zeros(pb.n_families)
    for k, pk in enumerate(probs):
        P = mats[k]
        B, Fp = GR._up(pb, P, leafv, float)
        O = [None] * n
        O[root], _ = GR._root_weight(pb, pr, B[root], "sum", False)
        Z += pk * (O[root] * B[root]).sum(axis=0)
        for p in range(n - 1, -1, -1):                       # parents before children
            if pb.leaf_taxon[p] >= 0:
                continue
            top = R if p == root else M
            for v in ch[p]:
                G = O[p].copy()
                for s in ch[p]:
                    if s != v or (mutant == "own_factor_left_in" and pb.leaf_taxon[v] >= 0):
                        G = G * Fp[s]
                Pv = P[v][:top + 1, :M + 1]
                if pb.leaf_taxon[v] < 0:
                    O[v] = Pv.T @ G
                    continue
                Ol = Pv[1:].T @ G[1:] if mutant == "row0_dropped" else Pv.T @ G
                if mutant == "mixed_after_normalising":
                    wk = _observe(pr, M, Ol)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        u[v] += pk * wk / wk.sum(axis=0)     # already observed: taken as w below
                else:
                    u[v] += pk * Ol
    if mutant == "mixed_after_normalising":
        return u, Z
    return [None if x is None else _observe(pr, M, x, at_c=mutant == "err_indexed_at_c") for x in u], Z


def _weights_brute(pb, pr, mats, leafv):
    n, M = pb.n_nodes, pb.max_family_size
    w = [None] * n
    ones = np.ones(pb.n_families)
    for v in range(n):
        if pb.leaf_taxon[v] < 0:
            continue
        w[v] = np.zeros((M + 1, pb.n_families))
        for y in range(M + 1):
            lv = dict(leafv)
            lv[v] = np.outer(count_vector(pr, M, y), ones)
            w[v][y] = _prune(pb, pr, mats, lv)
    return w, _prune(pb, pr, mats, leafv)


def reference(pb, pr, mats, route="updown", mutant=None):
    """dict: mean, sd, p_below, p_obs, p_above [F][n_taxa] (columns as pb.counts; NaN for a cell without mass), log_evidence,
    failed [F], and W, w_obs, cancel_sd [F][n_taxa]: the total, w at the observed count and 1 + (mean - x)^2 / var (1 where var
    is 0)."""
    assert mutant is None or mutant in MUTANTS, mutant
    assert route in ("updown", "brute") and (mutant is None or route == "updown")
    M, F, nt = pb.max_family_size, pb.n_families, pb.counts.shape[1]
    leafv = GR.leaf_vectors(pb, pr)
    w, Z = _weights_updown(pb, pr, mats, leafv, mutant) if route == "updown" else _weights_brute(pb, pr, mats, leafv)
    out = {k: np.full((F, nt), np.nan) for k in KEYS + ("W", "w_obs", "cancel_sd")}
    y = np.arange(M + 1)[:, None]
    fam = np.arange(F)
    for v in range(pb.n_nodes):
        if w[v] is None:
            continue
        t = int(pb.leaf_taxon[v])
        x = pb.counts[:, t].astype(np.int64)
        W = w[v].sum(axis=0)
        d = y - x[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = (y * w[v]).sum(axis=0) / W
            var = ((y - mean[None, :]) ** 2 * w[v]).sum(axis=0) / W
            cols = {"mean": mean, "sd": np.sqrt(var), "p_obs": w[v][x, fam] / W, "p_above": np.where(d > 0, w[v], 0.0).sum(axis=0) / W,
                    "p_below": np.where((d <= 0) if mutant == "below_includes_x" else (d < 0), w[v], 0.0).sum(axis=0) / W,
                    "cancel_sd": np.where(var > 0, 1 + (mean - x) ** 2 / var, 1.0)}
        bad = ~((W > 0) & np.isfinite(W))
        for key, val in cols.items():
            out[key][:, t] = np.where(bad, np.nan, val)
        out["W"][:, t] = W
        out["w_obs"][:, t] = w[v][x, fam]
    failed = ~((Z > 0) & np.isfinite(Z))
    out["failed"] = failed.astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["log_evidence"] = np.where(failed, np.nan, np.log(Z))
    out["Z"] = Z
    return out


def worst_cancellation(ref):
    """The largest factor by which rounding is amplified in any output: 1 + (mean - x)^2 / var for sd; mean and the three
    probabilities are sums of non-negative terms (factor 1)."""
    c = ref["cancel_sd"]
    return max(1.0, float(np.nanmax(c))) if np.any(~np.isnan(c)) else 1.0


def close(got, ref, c, label=""):
    """The project's rule: |got - ref| <= 1e-12 + 1e-10 c |ref| -- sd held to its own cancellation factor (at most c), the sums
    of non-negative terms to 1; the same NaN pattern; failed equal; log_evidence at 1e-12 + 1e-10 |ref|.  Prints the worst
    ratio before it asserts and returns it."""
    assert np.array_equal(np.asarray(got["failed"]), np.asarray(ref["failed"])), label
    worst = 0.0
    for key in KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape, (label, key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key)
        ok = ~np.isnan(r)
        if ok.any():
            factor = np.minimum(float(c), np.maximum(1.0, ref["cancel_sd"])) if key == "sd" else np.ones(r.shape)
            worst = max(worst, float((np.abs(g[ok] - r[ok]) / (1e-12 + 1e-10 * factor[ok] * np.abs(r[ok]))).max()))
    print("%s: worst |got - ref| / bound (c = %g) = %.3g" % (label, c, worst))
    assert worst <= 1.0, (label, worst)
    if "log_evidence" in got:
        ok = np.asarray(ref["failed"]) == 0
        g, r = np.asarray(got["log_evidence"]), np.asarray(ref["log_evidence"])
        assert np.all(np.isnan(g[~ok])) and np.all(np.abs(g[ok] - r[ok]) <= 1e-12 + 1e-10 * np.abs(r[ok])), label
    return worst
