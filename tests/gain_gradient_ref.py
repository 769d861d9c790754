"""Complex-step statement of cafe_gain_score_gradient (a helper, not a test): the gain prune of tests/gain_ref.py restated for
complex (alpha, beta, r) per branch -- row 0 by p_0 = (1 - beta)^r, p_k = p_{k-1} beta (r + k - 1) / k, rows by convolution with the
single-lineage law, then gain_ref's up pass and the sum rule -- at rates already on the 1e-9 grid, the imaginary part 1e-30 on ONE
parameter of ONE branch at a time: d = Im(log Z) / 1e-30.  Bumping alpha, beta or r gives d_alpha, d_beta, d_r; bumping lambda, mu or
nu inside one branch's key gives that branch's share d_v of the rate's score and with it c = sum_v |d_v| / |sum_v d_v|.  mus None:
mu = lambda, bumped together.  A saturated key's shares are exactly 0; a rate index with lambda_q = 0 has NaN."""
import numpy as np

import gain_posterior_ref as GP
import gain_ref as G
import gradient_ref as GR
import marginal_ref as MR

STEP = 1e-30
RATE_KEYS, BRANCH_KEYS = ("d_lambda", "d_mu", "d_nu"), ("d_alpha", "d_beta", "d_r")


def matrix(n, a, b, r, zero):
    P = np.zeros((n, n), dtype=complex)
    P[0, 0] = (1 - b) ** r
    for k in range(1, n):
        P[0, k] = P[0, k - 1] * b * (r + k - 1) / k
    one = np.concatenate([[a], (1 - a) * (1 - b) * b ** np.arange(n - 1)])
    for s in range(1, 1 if zero else n):
        P[s] = np.convolve(P[s - 1], one)[:n]
    return P


def table(pb, families, lambdas, mus, nus, prior, root_absent, error_model=None):
    """{lnl [n], d_lambda / d_mu / d_nu [n][n_lambdas] with cancel_<key>, d_alpha / d_beta / d_r [n][n_nodes]}"""
    nn, nl, n, root = pb.n_nodes, pb.n_lambdas, len(families), MR.root_of(pb)
    mass = GP.root_mass(prior, root_absent, pb.max_root_family_size)
    counts = [np.zeros(pb.n_taxa, dtype=np.int64) if f < 0 else pb.counts[f] for f in families]
    abr = lambda lq, mq, nq, t: GR.alpha_beta(lq, mq, t) + (nq / lq,)      # (alpha, beta, r) of a key whose rates may be complex
    keys, base, zero, built = {}, {}, {}, [None] * nn
    for v in range(nn):
        if v == root:
            continue
        i = int(pb.lambda_index[v])
        lq = G.quantize(lambdas[i])
        keys[v] = (lq, lq if mus is None else G.quantize(mus[i]), G.quantize(nus[i]), int(float(pb.branch_length[v]) * 1000) / 1000.0)
        if lq > 0:
            base[v] = abr(*keys[v])
            zero[v] = GR.is_zero(base[v][0], base[v][1])
        built[v] = matrix(pb.matrix_size, *base[v], zero[v]) if lq > 0 else G.matrix(pb.matrix_size, *keys[v]).astype(complex)

    def log_z(v=None, bumped=None):
        mats = list(built)
        if v is not None:
            mats[v] = matrix(pb.matrix_size, *bumped, False)
        return np.array([np.log(np.sum(mass * G.root_likelihoods(pb, c, mats, error_model))) for c in counts])

    out = {"lnl": log_z().real}
    out.update({k: np.zeros((n, nl)) for k in RATE_KEYS if mus is not None or k != "d_mu"})
    out.update({k: np.full((n, nn), np.nan) for k in BRANCH_KEYS})
    total = {k: np.zeros((n, nl)) for k in out if k in RATE_KEYS}
    for v, (lq, mq, nq, t) in keys.items():
        i, h = int(pb.lambda_index[v]), 1j * STEP
        if v not in base:
            for k in total:
                out[k][:, i] = np.nan
            continue
        for p, k in enumerate(BRANCH_KEYS):
            out[k][:, v] = 0.0 if zero[v] else log_z(v, [x + h * (p == j) for j, x in enumerate(base[v])]).imag / STEP
        bumps = {"d_lambda": (lq + h, mq + h if mus is None else mq, nq), "d_mu": (lq, mq + h, nq), "d_nu": (lq, mq, nq + h)}
        for k in total if not zero[v] else ():
            d = log_z(v, abr(*bumps[k], t)).imag / STEP
            out[k][:, i] += d
            total[k][:, i] += np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        out.update({"cancel_" + k: np.where(total[k] > 0, total[k] / np.abs(out[k]), 1.0) for k in total})
    return out
