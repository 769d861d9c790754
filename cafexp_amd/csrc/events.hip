// Expected gene gains and losses per branch: the posterior expectation, given the leaf counts, of the number of births and of
// deaths on the branch above every node.
//
// Tag every birth with a factor r and every death with a factor w.  The single-lineage generating function stays
// linear-fractional, phi(z) = a + c z / (1 - b z), and E[births; X_t = j | X_0 = i] = d P_ij / d r at r = w = 1 (deaths: d / d w).
// So the call is cafe_score_gradient's contraction (gradient.hip) of the branch joint G_v P_v B_v under the sum rule, in another
// direction of differentiation.  The one new ingredient: c, which the matrices carry as (1 - a)(1 - b), moves on its own.  With
// H the causal filter y[j] = x[j] + b y[j-1] and S the shift by one, along a row,
//     dP/da [i] = i P[i-1],        dP/dc [i] = i H S P[i-1],        dP/db [i] = i c H H S S P[i-1],
// lower triangular all three, so they hold on the matrix cut at M.  Transposed onto a panel, one anti-causal pass per column,
//     w1[j] = B[j] + b w1[j+1],    w2[j] = w1[j] + b w2[j+1],    Bt[j] = da B[j] + dc w1[j+1] + db c w2[j+2],
// gives the scanned panels of both tags at once; Ft = P_v Bt is the up pass's GEMM and the branch adds sum_{i >= 1} i G_v[i] Ft[i-1]
// to its own slot.  A leaf branch filters the rows of its row-major matrix into two scratch matrices and sums them against G at
// the taps of the observed count.  The six coefficients are non-negative, so nothing cancels.  The sums are kept per
// (tag, node); categories add into the same slot with weight p_k and the finish divides by Z = sum_k p_k Z_k.
// The root, weighted-dot, leaf-sum and finish kernels are gradient.hip's, behind its host launches (sum_product.h).
#include <cmath>
#include <string>
#include <vector>

#include "sum_product.h"

namespace cafe {

// {da, db, dc} of the births tag, then of the deaths tag, at r = w = 1; plain doubles in.  With s = lambda + mu,
// omega = |lambda - mu|, x = omega t / 2, sh = sinh(x) / omega, ch = cosh(x), T = s sh + ch (so a = 2 mu sh / T, b = 2 lambda sh / T
// and c = 1 / T^2) and d D / d r = d D / d w = -4 lambda mu for D = omega^2:
//     da/dr = mu W        db/dr = 2 lambda sh / T + lambda W        W = 2 lambda mu t^3 g(omega t) / T^2,  g(y) = (sinh y - y) / y^3
//     da/dw = 2 mu sh / T + mu W        db/dw = lambda W
//     dc/dr = dc/dw = 8 lambda mu (s sh' + ch') / T^3,        ch' = t sh / 4,  sh' = (t ch / 4 - sh / 2) / D
// -- sums of non-negative terms.  g and sh' are even and analytic in omega (limits 1/6 and t^3 / 48): series where omega t is
// small, so mu -> lambda is the plain limit; sh, ch and T carry e^-x each so that nothing overflows.
void bd_rates_events(double lambda, double mu, double t, double out[6]) {
    const double om = std::fabs(lambda - mu), s = lambda + mu, x = 0.5 * om * t, y = om * t;
    const double E = std::exp(-x);
    const double sh = 0.5 * t * (x > 0 ? -std::expm1(-2 * x) / (2 * x) : 1.0);       // sinh(x) / omega  e^-x
    const double ch = 0.5 * (1 + std::exp(-2 * x));                                  // cosh(x)  e^-x
    const double T = s * sh + ch;
    double g;                                                                         // g(y) e^-y
    if (y < 2) {                                             // sum_k y^2k / (2k+3)!: 16 terms reach 1e-22
        double term = 1.0 / 6, sum = 0.0;
        for (int k = 0; k < 16; ++k) { sum += term; term *= y * y / ((2 * k + 4) * (2 * k + 5)); }
        g = sum * std::exp(-y);
    } else {
        g = (-0.5 * std::expm1(-2 * y) - y * std::exp(-y)) / (y * y * y);
    }
    double shp;                                                                       // sh'  e^-x
    if (x < 1) {                                             // t^3 / 8 sum_{k >= 1} k x^(2k-2) / (2k+1)!
        double term = 1.0 / 6, sum = 0.0;
        for (int k = 1; k <= 16; ++k) { sum += k * term; term *= x * x / ((2 * k + 2) * (2 * k + 3)); }
        shp = 0.125 * t * t * t * sum * E;
    } else {
        shp = (0.25 * t * ch - 0.5 * sh) / (om * om);
    }
    const double chp = 0.25 * t * sh;
    const double W = 2 * lambda * mu * t * t * t * g / (T * T);
    const double dc = 8 * lambda * mu * (s * shp + chp) / (T * T * T) * E * E;
    out[0] = mu * W;
    out[1] = 2 * lambda * sh / T + lambda * W;
    out[2] = dc;
    out[3] = 2 * mu * sh / T + mu * W;
    out[4] = lambda * W;
    out[5] = dc;
}

namespace {

// ---------------------------------------------------------------------------------------------------------- kernels
// Both scanned panels of a branch in one pass over the rows 0..M of B, walked from M down: w1[j] = B[j] + beta w1[j+1],
// w2[j] = w1[j] + beta w2[j+1], Bt[q][j] = ca[q] B[j] + cc[q] w1[j+1] + cb[q] w2[j+2], q = 0 (gains), 1 (losses).  One thread per
// column; eight rows are loaded ahead of the recurrence that consumes them.
struct ScanCoeffs { double ca[2], cb[2], cc[2]; };
__global__ __launch_bounds__(256) void events_scan_kernel(const double* __restrict__ B, int M, int64_t ld, double beta, const ScanCoeffs k,
                                                          double* __restrict__ Bt0, double* __restrict__ Bt1) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double w1 = 0.0, w2 = 0.0, w2n = 0.0;                    // w1[j+1], w2[j+1], w2[j+2]
    for (int j0 = M; j0 >= 0; j0 -= 8) {
        double b[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) b[q] = j0 - q >= 0 ? B[(int64_t)(j0 - q) * ld + f] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (j0 - q < 0) break;
            const int64_t o = (int64_t)(j0 - q) * ld + f;
            Bt0[o] = k.ca[0] * b[q] + k.cc[0] * w1 + k.cb[0] * w2n;
            Bt1[o] = k.ca[1] * b[q] + k.cc[1] * w1 + k.cb[1] * w2n;
            w1 = b[q] + beta * w1;
            w2n = w2;
            w2 = w1 + beta * w2;
        }
    }
}

// The event rows of a row-major leaf matrix: dP[q][i][c] = i (ca[q] x[c] + cc[q] y1[c] + cb[q] y2[c]) for i = 1..np, c = 0..M, with
// x = P[i-1], y1 = H S x, y2 = H S y1 along the row.  A block takes 64 rows; the matrix moves through LDS in tiles of 64 rows x
// 32 columns so that global memory is read and written in whole row segments while thread r carries the filters of row r.
constexpr int kFR = 64, kFC = 32;
struct FilterParams {
    const double* P;
    int ldp, np, M;
    double beta;
    ScanCoeffs k;
    double* dP[2];
};
__global__ __launch_bounds__(256) void events_leaf_filter_kernel(const FilterParams a) {
    __shared__ double tin[kFR][kFC + 1], t0[kFR][kFC + 1], t1[kFR][kFC + 1];
    const int tid = threadIdx.x;
    const int i0 = 1 + blockIdx.x * kFR;                     // output rows i0 .. i0 + 63, read from rows i0 - 1 ..
    double prev = 0.0, y1 = 0.0, y2 = 0.0;                   // x[c-1], y1[c-1], y2[c-1]
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
                y2 = y1 + a.beta * y2;                       // y1 still holds y1[c-1]
                y1 = prev + a.beta * y1;
                prev = x;
                t0[tid][cc] = fi * (a.k.ca[0] * x + a.k.cc[0] * y1 + a.k.cb[0] * y2);
                t1[tid][cc] = fi * (a.k.ca[1] * x + a.k.cc[1] * y1 + a.k.cb[1] * y2);
            }
        }
        __syncthreads();
        for (int e = tid; e < kFR * kFC; e += 256) {
            const int r = e / kFC, cc = e % kFC;
            const int i = i0 + r, c = c0 + cc;
            if (i > a.np || c > a.M) continue;
            a.dP[0][(int64_t)i * a.ldp + c] = t0[r][cc];
            a.dP[1][(int64_t)i * a.ldp + c] = t1[r][cc];
        }
    }
}

// beta, the zero mark and the coefficients of both scans of the branch above a node in one category, from the quantized key
// the call's matrices are built from: ca = da, cb = db c, cc = dc with c = (1 - alpha)(1 - beta)
struct BranchEvents {
    double beta;
    bool zero;
    ScanCoeffs k;
};
BranchEvents branch_events(const cafe_ctx* c, const double* lambdas, int v, double mult) {
    const int layout = c->leaf_taxon[v] >= 0 ? 0 : 1;
    const long tq = c->pair_tq[layout][c->pair_of[v]];
    long lq, mq;
    quantized_rates(lambdas, context_mus(c), c->lam_idx[v], mult, &lq, &mq);
    BranchEvents r{};
    double alpha;
    if (c->mus.empty()) {
        const SlotParam sp = slot_param(lq, tq);
        alpha = r.beta = sp.alpha;
        r.zero = sp.zero != 0;
    } else {
        const SlotParamLM sp = slot_param_lm(lq, mq, tq);
        alpha = sp.alpha; r.beta = sp.beta; r.zero = sp.zero != 0;
    }
    double d[6];
    bd_rates_events(double(lq) / 1000000000.0, double(mq) / 1000000000.0, double(tq) / 1000.0, d);
    const double cq = (1 - alpha) * (1 - r.beta);
    for (int q = 0; q < 2; ++q) { r.k.ca[q] = d[3 * q]; r.k.cb[q] = d[3 * q + 1] * cq; r.k.cc[q] = d[3 * q + 2]; }
    return r;
}

}  // namespace

int expected_events_impl(cafe_ctx* c, const cafe_params* pr, const cafe_events_out* out) {
    if (const int rc = check_call_args(c, "cafe_expected_events", pr, out)) return rc;
    if (const int rc = check_model_args(c, "cafe_expected_events", pr)) return rc;
    PosteriorCall pc;
    if (const int rc = open_posterior_call(c, pr, &pc)) return rc;
    pc.timer.on = c->profile != 0;
    hipStream_t s = pc.s;
    UpPanels& up = pc.up;
    const int M = c->M, R = c->R, rows = c->N, n = c->n_nodes, K = pc.K, nI = pc.nI;
    const bool gamma = pc.gamma;
    const int n_acc = 2 * n;

    // workspace per column: B, F and O of every interior node; G, the two scanned panels, Ft and the panel that takes the down
    // GEMM's second output; Z_k, the sums per (tag, node), Z and its logarithm.  (The two event matrices of a leaf branch do not
    // depend on the columns and are not panels: they come on top.)
    const size_t dbl_per_col = (size_t)3 * nI * rows + 5 * (size_t)rows + K + n_acc + 2;
    int64_t cols = 0;
    if (const int rc = column_chunk(c, dbl_per_col * sizeof(double),
                                    "cafe_expected_events: not enough device memory for the panels of " + std::to_string(nI) + " interior nodes", &cols))
        return rc;
    const int ldp = c->pool.ld;
    const size_t leaf_mat = (size_t)(std::max(M, R) + 1) * ldp;
    DevBuf wd, dleaf;
    if (hipMalloc(&wd.p, dbl_per_col * cols * sizeof(double)) != hipSuccess || alloc_constants(c, kNoPriorLogs, &pc) != hipSuccess ||
        hipMalloc(&dleaf.p, sizeof(double) * leaf_mat * 2) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "cafe_expected_events: cannot allocate the workspace (%lld columns)", (long long)cols);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemsetAsync(wd.p, 0, dbl_per_col * cols * sizeof(double), s));
    HIP_TRY(c, hipMemsetAsync(dleaf.p, 0, sizeof(double) * leaf_mat * 2, s));
    const int64_t pstride = (int64_t)rows * cols;
    double* d_O = up.place(wd.p, nI, pstride);
    double* d_G = d_O + (int64_t)nI * pstride;
    double* d_Bt[2] = {d_G + pstride, d_G + 2 * pstride};
    double* d_Ft = d_Bt[1] + pstride;
    double* d_S = d_Ft + pstride;                            // the down GEMM's posterior product: not read
    double* d_zk = d_S + pstride;                            // [K][cols]
    double* d_acc = d_zk + (int64_t)K * cols;                // [2][n_nodes][cols]
    double* d_Z = d_acc + (int64_t)n_acc * cols;
    double* d_lnl = d_Z + cols;
    double* d_dP[2] = {static_cast<double*>(dleaf.p), static_cast<double*>(dleaf.p) + leaf_mat};
    if (const int rc = upload_constants(c, pr, &pc)) return rc;

    std::vector<double> h_acc((size_t)n_acc * cols), h_Z(cols), h_lnl(cols);

    const std::vector<Branch> down = branches_down(c);
    for (int64_t f0 = 0; f0 < c->Fp; f0 += cols) {
        const int64_t ld = std::min<int64_t>(cols, c->Fp - f0);
        const unsigned gb = (unsigned)((ld + 255) / 256);
        HIP_TRY(c, hipMemsetAsync(d_acc, 0, sizeof(double) * (size_t)n_acc * cols, s));
        for (int k = 0; k < K; ++k) {
            const double pk = gamma ? pr->cat_probs[k] : 1.0, mult = gamma ? pr->multipliers[k] : 1.0;
            auto acc_of = [&](int v, int q) { return d_acc + ((int64_t)q * n + v) * cols; };
            if (const int rc = marginal_up_pass(c, up, k, f0, ld, s, pc.timer)) return rc;
            if (const int rc = launch_root_weights(c, s, up.panel(up.B, c->root), pc.prior, nullptr, R, ld, up.panel(d_O, c->root),
                                                   d_zk + (int64_t)k * cols, nullptr, CAFE_ROOT_SUM, 0))
                return rc;
            const double* filtered = nullptr;                // the leaf matrix whose event rows the scratch holds
            for (const Branch& b : down) {
                const int v = b.v, np = b.np;
                const bool leaf = c->leaf_taxon[v] >= 0;
                const BranchEvents br = branch_events(c, pr->lambdas, v, mult);
                if (leaf && br.zero) continue;               // a saturated branch adds nothing
                GemmParams g;
                if (const int rc = down_branch(c, up, d_O, d_G, b, k, pk, f0, ld, s, &g)) return rc;
                if (leaf) {
                    const double* P = leaf_matrix(c, v, k);
                    if (P != filtered) {
                        FilterParams fp{};
                        fp.P = P; fp.ldp = ldp; fp.np = std::max(M, R); fp.M = M; fp.beta = br.beta; fp.k = br.k;
                        fp.dP[0] = d_dP[0]; fp.dP[1] = d_dP[1];
                        CAFE_LAUNCH(c, events_leaf_filter_kernel, dim3((unsigned)((fp.np + kFR - 1) / kFR)), dim3(256), 0, s, fp);
                        filtered = P;
                    }
                    if (const int rc = launch_leaf_sums(c, s, d_G, np, ld, d_dP[0], d_dP[1], ldp, leaf_counts(c, v, f0), up.err, up.n_dev, M, pk,
                                                        acc_of(v, 0), acc_of(v, 1)))
                        return rc;
                    continue;
                }
                g.out2 = d_S; g.first = 1;                   // the posterior product goes to a panel nobody reads
                if (const int rc = launch_gemm<kDown>(c, g, false, s, pc.timer)) return rc;
                if (br.zero) continue;
                CAFE_LAUNCH(c, events_scan_kernel, dim3(gb), dim3(256), 0, s, (const double*)up.panel(up.B, v), M, ld, br.beta, br.k, d_Bt[0], d_Bt[1]);
                for (int q = 0; q < 2; ++q) {
                    GemmParams u{};
                    u.Pt = g.Pt; u.ldp = g.ldp; u.X = d_Bt[q]; u.ld = ld; u.nr = np; u.nk = M + 1;
                    u.out1 = d_Ft; u.out2 = d_Ft;            // a plain store, twice
                    if (const int rc = launch_gemm<kUp>(c, u, false, s, pc.timer)) return rc;
                    if (const int rc = launch_weighted_dot(c, s, d_G, d_Ft, np, ld, pk, acc_of(v, q))) return rc;
                }
            }
        }
        if (const int rc = launch_finish_sums(c, s, d_zk, pc.probs, K, ld, cols, nullptr, d_acc, n_acc, d_Z, d_lnl)) return rc;
        HIP_TRY(c, hipMemcpyAsync(h_acc.data(), d_acc, sizeof(double) * (size_t)n_acc * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_Z.data(), d_Z, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_lnl.data(), d_lnl, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for_each_family_of_chunk(c, f0, ld, [&](int64_t f, int64_t col) {
            const bool bad = evidence_failed(h_Z[col]);
            if (out->log_evidence) out->log_evidence[f] = bad ? kNaN : h_lnl[col];
            if (out->failed) out->failed[f] = bad ? 1 : 0;
            for (int q = 0; q < 2; ++q) {
                double* dst = q == 0 ? out->gains : out->losses;
                if (!dst) continue;
                for (int v = 0; v < n; ++v) dst[f * n + v] = bad || v == c->root ? kNaN : h_acc[((size_t)q * n + v) * cols + col];
            }
        });
    }
    close_posterior_call(c, &pc.timer);
    return CAFE_OK;
}

}  // namespace cafe

extern "C" {

int cafe_expected_events(cafe_ctx* ctx, const cafe_params* params, const cafe_events_out* out) {
    return cafe::guarded_observed(ctx, "cafe_expected_events", [&] { return cafe::expected_events_impl(ctx, params, out); });
}

int cafe_bd_rates_events(double lambda, double mu, double t, double out[6]) {
    if (!out) return CAFE_ERR_ARGUMENT;
    const long lq = cafe::quantize_lambda(lambda), mq = cafe::quantize_lambda(mu), tq = cafe::quantize_time(t);
    cafe::bd_rates_events(double(lq) / 1000000000.0, double(mq) / 1000000000.0, double(tq) / 1000.0, out);
    return CAFE_OK;
}

}
