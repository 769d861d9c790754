"""Plain numpy statement of the scorer's sum rule and of the root posterior (a helper, not a test).

Built on marginal_ref's up pass: root_vectors gives L[f][k][j] = B_root[j + 1], the root vector of family f in category k
(inference_prune's return), from transition matrices mats[k][v] handed in.  From those:
  sum_rule        what cafe_score returns per family under CAFE_ROOT_SUM -- base model log sum_j L_j prior_j as a log-sum-exp
                  over t_j = log L_j + log prior_j, gamma model p_k sum_j L_j prior_j in the linear domain;
  root_posterior  what cafe_root_posterior returns: P(root = j + 1 | data_f) = sum_k p_k prior_j L^k_j / Z, its mean and first
                  arg max, the category posteriors p_k Z_k / Z, and total = the sum of the posteriors over every family of the
                  table that did not fail;
  em_step         the maximum-likelihood update of the root distribution, total / n_used, in doubles.
The prior is the float the ABI takes, widened to double, as the library reads it.  VARIANTS are deliberately WRONG
statements, for tests that ask whether their inputs can tell."""
import numpy as np

import marginal_ref as MR

VARIANTS = ("prior_shifted", "max_for_one_category", "cat_probs_forgotten", "multiplicities_forgotten", "failed_not_excluded")


def root_vectors(pb, pr, mats, families=None):
    """L[f][k][j], j = 0..R-1: the up pass of marginal_ref.updown_family, root sizes 1..R"""
    n, M, R = pb.n_nodes, pb.max_family_size, pb.max_root_family_size
    ch, root = MR.children_of(pb), MR.root_of(pb)
    fams = range(pb.n_families) if families is None else families
    out = np.zeros((len(fams), len(mats), R))
    for i, f in enumerate(fams):
        for k, P in enumerate(mats):
            B = [None] * n
            for v in range(n):                               # children before parents
                if pb.leaf_taxon[v] >= 0:
                    B[v] = MR.leaf_vector(pb, pr, f, v)
                    continue
                top = R if v == root else M
                b = np.ones(top + 1)
                for c in ch[v]:
                    b = b * (P[c][:top + 1, :M + 1] @ B[c])
                B[v] = b
            out[i, k] = B[root][1:R + 1]
    return out


def _prior(pr, prior=None):
    return np.asarray(pr.prior, dtype=np.float32).astype(np.float64) if prior is None else np.asarray(prior, dtype=np.float64)


def _probs(pr, K):
    return np.ones(K) if pr.cat_probs is None else np.asarray(pr.cat_probs, dtype=np.float64)


def log_sum_exp(t):
    """m + log sum exp(t - m); all -inf: -inf; a NaN term: NaN"""
    t = np.asarray(t, dtype=np.float64)
    if np.isnan(t).any():
        return np.nan
    m = t.max()
    if m == -np.inf:
        return -np.inf
    return float(m + np.log(np.exp(t - m).sum()))


def sum_rule(pr, L, variant=None, prior=None):
    """family_lnl [F]; with the gamma model also category_likelihood [F][K] and family_likelihood [F]"""
    assert variant is None or variant in VARIANTS, variant
    F, K, R = L.shape
    gamma = pr.multipliers is not None
    prior, probs = _prior(pr, prior), _probs(pr, K)
    if variant == "prior_shifted":
        prior = np.roll(prior, -1)
    if variant == "cat_probs_forgotten":
        probs = np.ones(K)
    res = {"family_lnl": np.empty(F)}
    if not gamma:
        with np.errstate(divide="ignore"):
            for f in range(F):
                res["family_lnl"][f] = log_sum_exp(np.log(L[f, 0]) + np.log(prior))
        return res
    cat = probs[None, :] * (L * prior[None, None, :]).sum(axis=2)
    if variant == "max_for_one_category":
        cat[:, K - 1] = probs[K - 1] * (L[:, K - 1] * prior[None, :]).max(axis=1)       # (the last: the likeliest on the tests' inputs)
    res["category_likelihood"] = cat
    res["family_likelihood"] = cat.sum(axis=1)
    with np.errstate(divide="ignore"):
        res["family_lnl"] = np.log(res["family_likelihood"])
    return res


def neg_lnl(family_lnl):
    """the call's value: minus the sum over the table; +inf when a family's value is -inf"""
    s = float(np.sum(family_lnl))
    return np.inf if s == -np.inf else -s


def root_posterior(pr, L, variant=None, prior=None, distinct=None):
    """L over EVERY family of the table (duplicates included).  distinct: the index of one representative per distinct family
    (only the variant that forgets the multiplicities reads it).  Returns total [R], n_used, mean, mode, mode_gap (relative gap
    of the two best masses), category_posterior [F][K], log_evidence, failed [F] and post [F][R]."""
    assert variant is None or variant in VARIANTS, variant
    F, K, R = L.shape
    prior, probs = _prior(pr, prior), _probs(pr, K)
    if variant == "prior_shifted":
        prior = np.roll(prior, -1)
    if variant == "cat_probs_forgotten":
        probs = np.ones(K)
    zk = (L * prior[None, None, :]).sum(axis=2)                              # [F][K]
    if variant == "max_for_one_category":
        zk[:, K - 1] = (L[:, K - 1] * prior[None, :]).max(axis=1)
    joint = prior[None, :] * np.einsum("k,fkj->fj", probs, L)               # [F][R]
    Z = (probs[None, :] * zk).sum(axis=1)
    failed = ~((Z > 0) & np.isfinite(Z))
    sizes = np.arange(1, R + 1)
    res = {"failed": failed.astype(np.int32), "Z": Z}
    with np.errstate(divide="ignore", invalid="ignore"):
        post = joint / Z[:, None]
        res["post"] = post
        res["mean"] = np.where(failed, np.nan, (post * sizes[None, :]).sum(axis=1))
        res["mode"] = np.where(failed, -1, 1 + np.argmax(joint, axis=1)).astype(np.int32)
        top = np.sort(joint, axis=1)[:, ::-1]
        res["mode_gap"] = np.where(failed | (R < 2), 1.0, (top[:, 0] - top[:, min(1, R - 1)]) / top[:, 0])
        res["category_posterior"] = np.where(failed[:, None], np.nan, probs[None, :] * zk / Z[:, None])
        if pr.multipliers is None:
            res["log_evidence"] = np.array([np.nan if failed[f] else log_sum_exp(np.log(L[f, 0]) + np.log(prior)) for f in range(F)])
        else:
            res["log_evidence"] = np.where(failed, np.nan, np.log(Z))
    rows = np.arange(F) if variant != "multiplicities_forgotten" else np.asarray(distinct)
    if variant == "failed_not_excluded":                     # their 0 / 0 rows enter the sum and they are counted
        res["total"] = post[rows].sum(axis=0)
        res["n_used"] = len(rows)
    else:
        keep = rows[~failed[rows]]
        res["total"] = post[keep].sum(axis=0)
        res["n_used"] = len(keep)
    return res


def em_step(pr, L, prior=None):
    """prior_new[j] = total[j] / n_used at the prior given (doubles; default: pr.prior)"""
    rp = root_posterior(pr, L, prior=prior)
    return rp["total"] / rp["n_used"]


def log_likelihood(pr, L, prior):
    """sum_f log sum_k p_k sum_j prior_j L^k_j over the families with a positive likelihood, prior in doubles"""
    F, K, R = L.shape
    z = (_probs(pr, K)[None, :] * (L * np.asarray(prior, dtype=np.float64)[None, None, :]).sum(axis=2)).sum(axis=1)
    return float(np.log(z[z > 0]).sum())


def bound(ref):
    """the project's bound for sums without cancellation (tests/test_marginal_gpu.py)"""
    return 1e-12 + 1e-10 * np.abs(ref)
