// Per-family score vectors: the derivative of every family's log likelihood in the rates.
//
// The model, the panels and the two passes are cafe_marginal_reconstruct's (marginal.hip): B_v and F_v from the up pass
// (sum_product.h), O_v and G_v = O_parent prod_{siblings} F_w from the down pass, so that for the branch above v
//     d Z / d theta = G_v^T (dP_v / d theta) B_v.
// Row i of P is the i-fold convolution of the single-lineage law, generating function ((a + (1-a-b) z) / (1 - b z))^i with
// a = alpha, b = beta of the branch (cafe_bd_rates).  With H the causal filter y[j] = x[j] + b y[j-1], S the shift by one and
// D = I - S, all acting along a row,
//     dP/da [i] = i H D P[i-1],        dP/db [i] = -i (1-a) H H S D P[i-1],
// and since the three operators are lower triangular this holds on the matrix cut at M as it stands.  So no derivative
// matrix is built: for a free rate theta of the branch the transposed operators are applied to B_v,
//     Bt = (da/dtheta) D^T H^T B_v - (db/dtheta)(1-a) D^T S^T H^T H^T B_v        (two anti-causal scans down a panel),
// one more GEMM of the up pass's form gives Ft = P_v Bt, and the branch adds sum_{i >= 1} i G_v[i] Ft[i-1].  A leaf branch
// needs dP/dtheta at the taps of the observed count only: the causal filters run along the rows of the row-major leaf matrix
// into a scratch matrix, and a kernel shaped like marginal_leaf_kernel sums it against G.
// The root weight O_root is the prior (CAFE_ROOT_SUM: Z is cafe_marginal_reconstruct's evidence) or the prior at the first
// arg max of a category and zero elsewhere (CAFE_ROOT_MAX: Z is what cafe_score takes the logarithm of).
// Gamma model: the sums are kept per (category, rate index, rate) and combined on the host,
//     d/d lambda_q = sum_k m_k d/d(lambda_q m_k),      d/d m_k = sum_q lambda_q d/d(lambda_q m_k) + mu_q d/d(mu_q m_k).
#include <cmath>
#include <vector>

#include "sum_product.h"

namespace cafe {

// phi1(x) = (e^x - 1) / x and phi2(x) = (e^x - 1 - x) / x^2, both times min(1, e^-x)
static void phi12_scaled(double x, double* s_out, double* p1, double* p2) {
    const double s = x > 0 ? std::exp(-x) : 1.0;
    double f1, f2;
    if (std::fabs(x) < 0.5) {                                // series: no cancellation, 20 terms reach 1e-19
        double t1 = 1.0, t2 = 0.5;
        f1 = 1.0; f2 = 0.5;
        for (int k = 1; k <= 20; ++k) {
            t1 *= x / (k + 1);
            t2 *= x / (k + 2);
            f1 += t1; f2 += t2;
        }
        f1 *= s; f2 *= s;
    } else if (x > 0) {
        const double em = -std::expm1(-x);                   // 1 - e^-x
        f1 = em / x;
        f2 = (em - x * s) / (x * x);
    } else {
        const double e = std::expm1(x);
        f1 = e / x;
        f2 = (e - x) / (x * x);
    }
    *s_out = s; *p1 = f1; *p2 = f2;
}

// d alpha / d lambda, d alpha / d mu, d beta / d lambda, d beta / d mu of bd_rates(lambda, mu, t) (cafe_kernels.h), plain
// doubles in.  With x = (lambda - mu) t, E = e^x, Q = (1 + lambda t phi1)^2:
//     da/dl = -mu E t^2 phi2 / Q            da/dm = E (t + lambda t^2 phi2) / Q
//     db/dl = (t + t^2 (lambda phi1 - mu phi2)) / Q        db/dm = lambda t^2 (phi2 - phi1) / Q
// -- no division by lambda - mu, so mu -> lambda is the plain limit; for x > 0 numerator and denominator carry e^-x each so
// that nothing overflows.
void bd_rates_grad(double lambda, double mu, double t, double out[4]) {
    const double x = (lambda - mu) * t;
    double s, f1, f2;
    phi12_scaled(x, &s, &f1, &f2);
    if (x > 0) {                                             // f1 = phi1 e^-x, f2 = phi2 e^-x, Q e^-2x
        const double q = s + lambda * t * f1, Q = q * q;
        out[0] = -mu * t * t * f2 / Q;
        out[1] = (t * s + lambda * t * t * f2) / Q;
        out[2] = (t * s * s + t * t * s * (lambda * f1 - mu * f2)) / Q;
        out[3] = lambda * t * t * s * (f2 - f1) / Q;
    } else {
        const double E = std::exp(x), q = 1 + lambda * t * f1, Q = q * q;
        out[0] = -mu * E * t * t * f2 / Q;
        out[1] = E * (t + lambda * t * t * f2) / Q;
        out[2] = (t + t * t * (lambda * f1 - mu * f2)) / Q;
        out[3] = lambda * t * t * (f2 - f1) / Q;
    }
}

namespace {

// ---------------------------------------------------------------------------------------------------------- kernels
// Root of one category: O_root[s] and Z_k = sum_s O_root[s] B_root[s].  rule 1 (sum): O_root[s] = prior[s-1].  rule 0 (max):
// the prior at the first arg max of B_root[s] prior[s-1] -- of log B_root[s] + log prior[s-1] when use_log, the comparison
// root_reduce_kernel makes for the base model, whose maximum goes to lbest -- and zero elsewhere.  A NaN at s = 1 stays, a
// NaN elsewhere never wins a comparison (the scorer's scan).
__global__ __launch_bounds__(256) void gradient_root_kernel(const double* __restrict__ B, const double* __restrict__ prior, const double* __restrict__ logprior,
                                                            int R, int64_t ld, double* __restrict__ O, double* __restrict__ zk, double* __restrict__ lbest,
                                                            int rule, int use_log) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    O[f] = 0.0;
    if (rule == 1) {
        double z = 0.0;
        for (int s = 1; s <= R; ++s) {
            const double w = prior[s - 1];
            O[(int64_t)s * ld + f] = w;
            z += w * B[(int64_t)s * ld + f];
        }
        zk[f] = z;
        return;
    }
    double best = 0.0;
    int arg = 1;
    for (int s = 1; s <= R; ++s) {
        const double b = B[(int64_t)s * ld + f];
        const double val = use_log ? log(b) + logprior[s - 1] : b * prior[s - 1];
        if (s == 1 || val > best) { best = val; arg = s; }
    }
    for (int s = 1; s <= R; ++s) O[(int64_t)s * ld + f] = s == arg ? prior[s - 1] : 0.0;
    zk[f] = B[(int64_t)arg * ld + f] * prior[arg - 1];
    if (use_log) lbest[f] = best;
}

// Bt = ca D^T H^T B - cb D^T S^T H^T H^T B over the rows 0..M of a panel, walked from M down: w1[j] = B[j] + beta w1[j+1],
// w2[j] = w1[j] + beta w2[j+1], u[j] = ca w1[j] - cb w2[j+1], Bt[j] = u[j] - u[j+1].  One thread per column; eight rows are
// loaded ahead of the recurrence that consumes them.
__global__ __launch_bounds__(256) void gradient_scan_kernel(const double* __restrict__ B, int M, int64_t ld, double beta, double ca, double cb,
                                                            double* __restrict__ Bt) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double w1 = 0.0, w2 = 0.0, un = 0.0;
    for (int j0 = M; j0 >= 0; j0 -= 8) {
        double b[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) b[q] = j0 - q >= 0 ? B[(int64_t)(j0 - q) * ld + f] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (j0 - q < 0) break;
            w1 = b[q] + beta * w1;
            const double u = ca * w1 - cb * w2;              // w2 still holds w2[j+1]
            w2 = w1 + beta * w2;
            Bt[(int64_t)(j0 - q) * ld + f] = u - un;
            un = u;
        }
    }
}

// acc[f] += pk sum_{i = 1..np} i G[i][f] Ft[i-1][f], in the order of i; the same sum times pk2 into acc2 when there is one
// (cafe_branch_scores: the branch's own row)
__global__ __launch_bounds__(256) void gradient_dot_kernel(const double* __restrict__ G, const double* __restrict__ Ft, int np, int64_t ld, double pk,
                                                           double* __restrict__ acc, double pk2, double* __restrict__ acc2) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double s = 0.0;
#pragma unroll 8
    for (int i = 1; i <= np; ++i) s += (double)i * G[(int64_t)i * ld + f] * Ft[(int64_t)(i - 1) * ld + f];
    acc[f] += pk * s;
    if (acc2) acc2[f] += pk2 * s;
}

// The derivative rows of a row-major leaf matrix: dP[p][i][c] = i (ca[p] y[c] - cb[p] z[c-1]) for i = 1..np, c = 0..M, with
// y = H D P[i-1], z = H y along the row.  A block takes 64 rows; the matrix moves through LDS in tiles of 64 rows x 32 columns
// so that global memory is read and written in whole row segments while thread r carries the filters of row r.
constexpr int kFR = 64, kFC = 32;
struct FilterParams {
    const double* P;
    int ldp, np, M, n_par;
    double beta, ca[2], cb[2];
    double* dP[2];
};
__global__ __launch_bounds__(256) void gradient_leaf_filter_kernel(const FilterParams a) {
    __shared__ double tin[kFR][kFC + 1], t0[kFR][kFC + 1], t1[kFR][kFC + 1];
    const int tid = threadIdx.x;
    const int i0 = 1 + blockIdx.x * kFR;                     // output rows i0 .. i0 + 63, read from rows i0 - 1 ..
    double prev = 0.0, y = 0.0, z = 0.0;
    for (int c0 = 0; c0 <= a.M; c0 += kFC) {
        __syncthreads();
        for (int e = tid; e < kFR * kFC; e += 256) {
            const int r = e / kFC, cc = e % kFC;
            const int i = i0 + r, c = c0 + cc;
            tin[r][cc] = (i <= a.np && c <= a.M) ? a.P[(int64_t)(i - 1) * a.ldp + c] : 0.0;
        }
        __syncthreads();
        if (tid < kFR) {
            const double fi = (double)(i0 + tid);
            for (int cc = 0; cc < kFC; ++cc) {
                const double x = tin[tid][cc];
                y = (x - prev) + a.beta * y;
                prev = x;
                t0[tid][cc] = fi * (a.ca[0] * y - a.cb[0] * z);
                t1[tid][cc] = fi * (a.ca[1] * y - a.cb[1] * z);      // z still holds z[c-1]
                z = y + a.beta * z;
            }
        }
        __syncthreads();
        for (int e = tid; e < kFR * kFC; e += 256) {
            const int r = e / kFC, cc = e % kFC;
            const int i = i0 + r, c = c0 + cc;
            if (i > a.np || c > a.M) continue;
            a.dP[0][(int64_t)i * a.ldp + c] = t0[r][cc];
            if (a.n_par > 1) a.dP[1][(int64_t)i * a.ldp + c] = t1[r][cc];
        }
    }
}

// A leaf branch: acc[p][f] += pk sum_t err[x][t] sum_{i = 1..np} G[i][f] dP[p][i][c_t], c_t the taps of the observed count x
// inside [0, M] (c = x without an error model), in the scorer's tap order; the same two sums times bk[p] into row[p] when there
// are any (cafe_branch_scores: the branch's own rows)
struct LeafRows { double bk[2]; double* row[2]; };
__global__ __launch_bounds__(256) void gradient_leaf_kernel(const double* __restrict__ G, int np, int64_t ld, const double* __restrict__ dP0,
                                                            const double* __restrict__ dP1, int ldp, const int32_t* __restrict__ cnt,
                                                            const double* __restrict__ err, int n_dev, int M, double pk, double* __restrict__ acc0,
                                                            double* __restrict__ acc1, const LeafRows rows) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const int x = cnt[f];
    const int n_tap = err ? n_dev : 1, half = err ? (n_dev - 1) / 2 : 0;
    double s0 = 0.0, s1 = 0.0;
    for (int t = 0; t < n_tap; ++t) {
        const int c = x - half + t;
        if (c < 0 || c > M) continue;
        const double w = err ? err[(int64_t)x * n_dev + t] : 1.0;
        double d0 = 0.0, d1 = 0.0;
        for (int i = 1; i <= np; ++i) {
            const double g = G[(int64_t)i * ld + f];
            d0 += g * dP0[(int64_t)i * ldp + c];
            if (dP1) d1 += g * dP1[(int64_t)i * ldp + c];
        }
        s0 += w * d0;
        s1 += w * d1;
    }
    acc0[f] += pk * s0;
    if (dP1) acc1[f] += pk * s1;
    if (rows.row[0]) rows.row[0][f] += rows.bk[0] * s0;
    if (rows.row[1]) rows.row[1][f] += rows.bk[1] * s1;
}

// Z = sum_k p_k Z_k in the order of k; lnl = log Z (or the base model's maximum of logarithms); every sum of the column
// divided by Z.  Z = 0 or not finite: NaN throughout.
__global__ __launch_bounds__(256) void gradient_finish_kernel(const double* __restrict__ zk, const double* __restrict__ probs, int K, int64_t ld, int64_t stride,
                                                              const double* __restrict__ lbest, double* __restrict__ acc, int n_acc,
                                                              double* __restrict__ Z, double* __restrict__ lnl) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double z = 0.0;
    for (int k = 0; k < K; ++k) z += probs[k] * zk[(int64_t)k * stride + f];
    Z[f] = z;
    const double nan = __builtin_nan("");
    const bool bad = evidence_failed(z);
    lnl[f] = bad ? nan : (lbest ? lbest[f] : log(z));
    for (int j = 0; j < n_acc; ++j) {
        double* o = acc + (int64_t)j * stride + f;
        *o = bad ? nan : *o / z;
    }
}

// alpha, beta, the zero mark and the derivatives in the call's free rates of the branch above a node in one category,
// from the quantized key the call's matrices are built from (fill_slots)
struct BranchRates {
    double alpha, beta;
    bool zero;
    double da[2], db[2];                 // [0]: lambda (or the common rate along lambda = mu), [1]: mu
};
BranchRates branch_rates(const cafe_ctx* c, const double* lambdas, int v, double mult) {
    const int layout = c->leaf_taxon[v] >= 0 ? 0 : 1;
    const long tq = c->pair_tq[layout][c->pair_of[v]];
    long lq, mq;
    quantized_rates(lambdas, context_mus(c), c->lam_idx[v], mult, &lq, &mq);
    BranchRates r{};
    const double l = double(lq) / 1000000000.0, m = double(mq) / 1000000000.0, t = double(tq) / 1000.0;
    if (c->mus.empty()) {
        const SlotParam sp = slot_param(lq, tq);
        r.alpha = r.beta = sp.alpha;
        r.zero = sp.zero != 0;
        r.da[0] = r.db[0] = t / ((1 + l * t) * (1 + l * t));
        return r;
    }
    const SlotParamLM sp = slot_param_lm(lq, mq, tq);
    r.alpha = sp.alpha; r.beta = sp.beta; r.zero = sp.zero != 0;
    double g[4];
    bd_rates_grad(l, m, t, g);
    r.da[0] = g[0]; r.da[1] = g[1]; r.db[0] = g[2]; r.db[1] = g[3];
    return r;
}

}  // namespace

// The kernels cafe_expected_events (events.hip) contracts the same branch joint with, behind host launches (sum_product.h)
int launch_root_weights(cafe_ctx* c, hipStream_t s, const double* B, const double* prior, const double* logprior, int R, int64_t ld, double* O, double* zk,
                        double* lbest, int rule, int use_log) {
    CAFE_LAUNCH(c, gradient_root_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, s, B, prior, logprior, R, ld, O, zk, lbest, rule, use_log);
    return CAFE_OK;
}
int launch_weighted_dot(cafe_ctx* c, hipStream_t s, const double* G, const double* Ft, int np, int64_t ld, double pk, double* acc) {
    CAFE_LAUNCH(c, gradient_dot_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, s, G, Ft, np, ld, pk, acc, 0.0, (double*)nullptr);
    return CAFE_OK;
}
int launch_leaf_sums(cafe_ctx* c, hipStream_t s, const double* G, int np, int64_t ld, const double* dP0, const double* dP1, int ldp, const int32_t* cnt,
                     const double* err, int n_dev, int M, double pk, double* acc0, double* acc1) {
    CAFE_LAUNCH(c, gradient_leaf_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, s, G, np, ld, dP0, dP1, ldp, cnt, err, n_dev, M, pk, acc0, acc1, LeafRows{});
    return CAFE_OK;
}
int launch_finish_sums(cafe_ctx* c, hipStream_t s, const double* zk, const double* probs, int K, int64_t ld, int64_t stride, const double* lbest, double* acc,
                       int n_acc, double* Z, double* lnl) {
    CAFE_LAUNCH(c, gradient_finish_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, s, zk, probs, K, ld, stride, lbest, acc, n_acc, Z, lnl);
    return CAFE_OK;
}

// The walk of cafe_score_gradient.  cafe_branch_scores (branch_scores.hip) takes it too, with a score panel `sp`: every dot
// and leaf sum then also goes, weighted p_k m_k lambda_q (or mu_q) -- the derivative in the logarithm of the branch's rate --
// into the branch's own row of the panel, and the global scores of every column go to the panel's last rows.  What the
// kernels add into the sums per lambda index, and in which order, does not depend on `sp`.
int gradient_walk(cafe_ctx* c, const char* entry, const cafe_params* pr, int32_t root_rule, const cafe_gradient_out* out, ScorePanel* sp) {
    if (const int rc = check_call_args(c, entry, pr, out)) return rc;
    if (root_rule != CAFE_ROOT_MAX && root_rule != CAFE_ROOT_SUM) { set_err(c, "%s: root_rule must be CAFE_ROOT_MAX or CAFE_ROOT_SUM", entry); return CAFE_ERR_ARGUMENT; }
    if (pr->model != CAFE_MODEL_GAMMA && out->d_multiplier) { set_err(c, "%s: d_multiplier needs the gamma model", entry); return CAFE_ERR_ARGUMENT; }
    if (const int rc = check_model_args(c, entry, pr)) return rc;
    if (out->d_mu && c->mus.empty()) { set_err(c, "%s: d_mu needs death rates (cafe_set_death_rates)", entry); return CAFE_ERR_STATE; }
    PosteriorCall pc;
    if (const int rc = open_posterior_call(c, pr, &pc)) return rc;
    pc.timer.on = c->profile != 0;
    hipStream_t s = pc.s;
    UpPanels& up = pc.up;
    const int M = c->M, R = c->R, rows = c->N, nl = c->n_lambdas, K = pc.K, nI = pc.nI;
    const int n_par = c->mus.empty() ? 1 : 2;
    const bool gamma = pc.gamma, use_log = !gamma && root_rule == CAFE_ROOT_MAX;
    const int n_acc = K * nl * n_par;
    const int n_glob = nl * n_par + (gamma ? K : 0);         // d_lambda, d_mu, d_multiplier of a column
    if (sp) if (const int rc = score_panel_open(c, entry, n_par, n_glob, sp)) return rc;      // before the batch is sized: it stays

    // workspace per column: B, F and O of every interior node; G, the scanned panel Bt, Ft and the panel that takes the down
    // GEMM's second output; Z_k, the sums, Z, lnl and the base model's maximum.  (The two derivative matrices of a leaf branch
    // do not depend on the columns and are not panels: they come on top.)
    const size_t dbl_per_col = (size_t)3 * nI * rows + 4 * (size_t)rows + K + n_acc + 3;
    int64_t cols = 0;
    if (const int rc = column_chunk(c, dbl_per_col * sizeof(double),
                                    std::string(entry) + ": not enough device memory for the panels of " + std::to_string(nI) + " interior nodes", &cols))
        return rc;
    const int ldp = c->pool.ld;
    const size_t leaf_mat = (size_t)(std::max(M, R) + 1) * ldp;
    DevBuf wd, dleaf;
    if (hipMalloc(&wd.p, dbl_per_col * cols * sizeof(double)) != hipSuccess || alloc_constants(c, kWithPriorLogs, &pc) != hipSuccess ||
        hipMalloc(&dleaf.p, sizeof(double) * leaf_mat * n_par) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "%s: cannot allocate the workspace (%lld columns)", entry, (long long)cols);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemsetAsync(wd.p, 0, dbl_per_col * cols * sizeof(double), s));
    HIP_TRY(c, hipMemsetAsync(dleaf.p, 0, sizeof(double) * leaf_mat * n_par, s));
    const int64_t pstride = (int64_t)rows * cols;
    double* d_O = up.place(wd.p, nI, pstride);
    double* d_G = d_O + (int64_t)nI * pstride;
    double* d_Bt = d_G + pstride;
    double* d_Ft = d_Bt + pstride;
    double* d_S = d_Ft + pstride;                            // the down GEMM's posterior product: not read
    double* d_zk = d_S + pstride;                            // [K][cols]
    double* d_acc = d_zk + (int64_t)K * cols;                // [K][n_lambdas][n_par][cols]
    double* d_Z = d_acc + (int64_t)n_acc * cols;
    double* d_lnl = d_Z + cols;
    double* d_lbest = d_lnl + cols;
    double* d_dP[2] = {static_cast<double*>(dleaf.p), n_par > 1 ? static_cast<double*>(dleaf.p) + leaf_mat : nullptr};
    if (const int rc = upload_constants(c, pr, &pc)) return rc;

    std::vector<double> h_acc((size_t)n_acc * cols), h_Z(cols), h_lnl(cols), h_glob((size_t)n_glob * cols);

    const std::vector<Branch> down = branches_down(c);
    for (int64_t f0 = 0; f0 < c->Fp; f0 += cols) {
        const int64_t ld = std::min<int64_t>(cols, c->Fp - f0);
        const unsigned gb = (unsigned)((ld + 255) / 256);
        HIP_TRY(c, hipMemsetAsync(d_acc, 0, sizeof(double) * (size_t)n_acc * cols, s));
        for (int k = 0; k < K; ++k) {
            const double pk = gamma ? pr->cat_probs[k] : 1.0, mult = gamma ? pr->multipliers[k] : 1.0;
            auto acc_of = [&](int v, int p) { return d_acc + (((int64_t)k * nl + c->lam_idx[v]) * n_par + p) * cols; };
            auto log_rate = [&](int v, int p) { return pk * (mult * (p == 0 ? pr->lambdas[c->lam_idx[v]] : c->mus[c->lam_idx[v]])); };
            if (const int rc = marginal_up_pass(c, up, k, f0, ld, s, pc.timer)) return rc;
            CAFE_LAUNCH(c, gradient_root_kernel, dim3(gb), dim3(256), 0, s, up.panel(up.B, c->root), pc.prior, pc.logprior, R, ld, up.panel(d_O, c->root),
                        d_zk + (int64_t)k * cols, d_lbest, (int)root_rule, use_log ? 1 : 0);
            const double* filtered = nullptr;                // the leaf matrix whose derivative rows the scratch holds
            for (const Branch& b : down) {
                const int v = b.v, np = b.np;
                const bool leaf = c->leaf_taxon[v] >= 0;
                const BranchRates br = branch_rates(c, pr->lambdas, v, mult);
                if (leaf && br.zero) continue;               // a saturated branch adds nothing
                GemmParams g;
                if (const int rc = down_branch(c, up, d_O, d_G, b, k, pk, f0, ld, s, &g)) return rc;
                if (leaf) {
                    const double* P = leaf_matrix(c, v, k);
                    if (P != filtered) {
                        FilterParams fp{};
                        fp.P = P; fp.ldp = ldp; fp.np = std::max(M, R); fp.M = M; fp.n_par = n_par; fp.beta = br.beta;
                        for (int q = 0; q < n_par; ++q) { fp.ca[q] = br.da[q]; fp.cb[q] = br.db[q] * (1 - br.alpha); fp.dP[q] = d_dP[q]; }
                        if (n_par == 1) fp.dP[1] = d_dP[0];
                        CAFE_LAUNCH(c, gradient_leaf_filter_kernel, dim3((unsigned)((fp.np + kFR - 1) / kFR)), dim3(256), 0, s, fp);
                        filtered = P;
                    }
                    LeafRows rows{};
                    for (int q = 0; sp && q < n_par; ++q) { rows.bk[q] = log_rate(v, q); rows.row[q] = score_panel_row(sp, v, q, f0); }
                    CAFE_LAUNCH(c, gradient_leaf_kernel, dim3(gb), dim3(256), 0, s, d_G, np, ld, d_dP[0], (const double*)d_dP[1], ldp,
                                leaf_counts(c, v, f0), up.err, up.n_dev, M, pk, acc_of(v, 0), n_par > 1 ? acc_of(v, 1) : nullptr, rows);
                    continue;
                }
                g.out2 = d_S; g.first = 1;                   // the posterior product goes to a panel nobody reads
                if (const int rc = launch_gemm<kDown>(c, g, false, s, pc.timer)) return rc;
                if (br.zero) continue;
                for (int q = 0; q < n_par; ++q) {
                    CAFE_LAUNCH(c, gradient_scan_kernel, dim3(gb), dim3(256), 0, s, (const double*)up.panel(up.B, v), M, ld, br.beta, br.da[q],
                                br.db[q] * (1 - br.alpha), d_Bt);
                    GemmParams u{};
                    u.Pt = g.Pt; u.ldp = g.ldp; u.X = d_Bt; u.ld = ld; u.nr = np; u.nk = M + 1;
                    u.out1 = d_Ft; u.out2 = d_Ft;            // a plain store, twice
                    if (const int rc = launch_gemm<kUp>(c, u, false, s, pc.timer)) return rc;
                    CAFE_LAUNCH(c, gradient_dot_kernel, dim3(gb), dim3(256), 0, s, (const double*)d_G, (const double*)d_Ft, np, ld, pk, acc_of(v, q),
                                sp ? log_rate(v, q) : 0.0, sp ? score_panel_row(sp, v, q, f0) : (double*)nullptr);
                }
            }
        }
        CAFE_LAUNCH(c, gradient_finish_kernel, dim3(gb), dim3(256), 0, s, (const double*)d_zk, pc.probs, K, ld, cols,
                    use_log ? (const double*)d_lbest : nullptr, d_acc, n_acc, d_Z, d_lnl);
        HIP_TRY(c, hipMemcpyAsync(h_acc.data(), d_acc, sizeof(double) * (size_t)n_acc * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_Z.data(), d_Z, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_lnl.data(), d_lnl, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        // the global scores of every column, then of every family that shares it
        for (int64_t col = 0; col < ld; ++col) {
            auto a = [&](int k, int q, int p) { return h_acc[(((size_t)k * nl + q) * n_par + p) * cols + col]; };
            for (int q = 0; q < nl; ++q) {
                double dl = 0.0, dm = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double m = gamma ? pr->multipliers[k] : 1.0;
                    dl += m * a(k, q, 0);
                    if (n_par > 1) dm += m * a(k, q, 1);
                }
                h_glob[(size_t)q * cols + col] = dl;
                if (n_par > 1) h_glob[(size_t)(nl + q) * cols + col] = dm;
            }
            for (int k = 0; gamma && k < K; ++k) {
                double d = 0.0;
                for (int q = 0; q < nl; ++q) {
                    d += pr->lambdas[q] * a(k, q, 0);
                    if (n_par > 1) d += c->mus[q] * a(k, q, 1);
                }
                h_glob[(size_t)(nl * n_par + k) * cols + col] = d;
            }
        }
        for_each_family_of_chunk(c, f0, ld, [&](int64_t f, int64_t col) {
            const bool bad = evidence_failed(h_Z[col]);
            if (out->family_lnl) out->family_lnl[f] = bad ? kNaN : h_lnl[col];
            if (out->failed) out->failed[f] = bad ? 1 : 0;
            for (int q = 0; q < nl; ++q) {
                if (out->d_lambda) out->d_lambda[f * nl + q] = bad ? kNaN : h_glob[(size_t)q * cols + col];
                if (out->d_mu) out->d_mu[f * nl + q] = bad ? kNaN : h_glob[(size_t)(nl + q) * cols + col];
            }
            if (out->d_multiplier)
                for (int k = 0; k < K; ++k) out->d_multiplier[f * K + k] = bad ? kNaN : h_glob[(size_t)(nl * n_par + k) * cols + col];
        });
        if (sp) if (const int rc = score_panel_batch(c, s, sp, f0, ld, cols, d_Z, h_Z.data(), h_glob.data())) return rc;
    }
    if (sp) if (const int rc = score_panel_close(c, s, sp)) return rc;
    close_posterior_call(c, &pc.timer);
    return CAFE_OK;
}

}  // namespace cafe

extern "C" {

int cafe_score_gradient(cafe_ctx* ctx, const cafe_params* params, int32_t root_rule, const cafe_gradient_out* out) {
    return cafe::guarded_observed(ctx, "cafe_score_gradient", [&] { return cafe::gradient_walk(ctx, "cafe_score_gradient", params, root_rule, out, nullptr); });
}

int cafe_bd_rates_grad(double lambda, double mu, double t, double out[4]) {
    if (!out) return CAFE_ERR_ARGUMENT;
    const long lq = cafe::quantize_lambda(lambda), mq = cafe::quantize_lambda(mu), tq = cafe::quantize_time(t);
    cafe::bd_rates_grad(double(lq) / 1000000000.0, double(mq) / 1000000000.0, double(tq) / 1000.0, out);
    return CAFE_OK;
}

}
