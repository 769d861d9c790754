// Marginal ancestral reconstruction: posterior size distributions of every node, credible intervals and the posterior
// probability that a branch expanded or contracted.
//
// The model is the scorer's (inference_prune / compute_node_probability, src/core.cpp:133, src/probability.cpp:173-242), not
// the joint reconstructor's variant with L[0] = 0.  With i = size of a node's parent, j = size of the node v, P_v its matrix:
//   up    F_v[i] = sum_j P_v[i][j] B_v[j]          B_p[i] = prod_{children} F_c[i]           leaf: the scorer's gather, taps included
//   root  O_root[s] = prior[s-1], s = 1..R         Z = sum_s O_root[s] B_root[s]
//   down  G_v[i] = O_p[i] prod_{siblings} F_w[i]   O_v[j] = sum_i P_v[i][j] G_v[i]            (products of stored factors: no division)
//   post_v[j] ~ O_v[j] B_v[j];  joint of a branch = G_v[i] P_v[i][j] B_v[j] / Z
// Panels are [size][family], families fastest.  The interior matrices are the k-major ones K1 builds (Pt[j][i-1] = P[i][j],
// row i = 0 of P is e_0 and is not stored), so ONE fp64 MFMA GEMM serves both passes: the up pass reads A[i][j] = Pt[j][i-1]
// (A transposed in memory), the down pass reads the rows of Pt as they lie.  Row 0 of P is added by the epilogue, as K5 does.
// Gamma model: every category runs the same launches; the un-normalised posteriors are accumulated with weight cat_probs[k]
// in one panel per interior node and summarised once (the base model is K = 1).
#include <cmath>
#include <vector>

#include "sum_product.h"

namespace cafe {

namespace {

// root weighting: O_root[s] = prior[s-1], acc_root[s] (+)= p_k prior[s-1] B_root[s], s = 1..R; row 0 carries no mass
__global__ __launch_bounds__(256) void marginal_root_kernel(const double* __restrict__ B, const double* __restrict__ prior, int R, int64_t ld,
                                                            double* __restrict__ O, double* __restrict__ acc, double pk, int first) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const int s0 = blockIdx.y * 16, s1 = min(R + 1, s0 + 16);
    for (int s = s0; s < s1; ++s) {
        const int64_t o = (int64_t)s * ld + f;
        const double w = s >= 1 ? prior[s - 1] : 0.0;
        O[o] = w;
        const double t = pk * (w * B[o]);
        acc[o] = first ? t : acc[o] + t;
    }
}

// out[f] (+)= p_k sum_j D[j][f]: the masked down GEMM dotted with B_v (its epilogue already multiplied)
__global__ __launch_bounds__(256) void marginal_colsum_kernel(const double* __restrict__ D, int rows, int64_t ld, double* __restrict__ out, double pk, int first) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double s = 0.0;
    for (int j = 0; j < rows; ++j) s += D[(int64_t)j * ld + f];
    out[f] = first ? pk * s : out[f] + pk * s;
}

// A leaf branch: for every tap c of the observed count x (c = x without an error model), sum_i G[i] P[i][c] split at i < c,
// i = c, i > c.  acc[t] (+)= p_k e[t] (whole sum): the posterior over the taps; acc[n_tap] / acc[n_tap + 1]: the mass with
// the leaf above / below its parent.
__global__ __launch_bounds__(256) void marginal_leaf_kernel(const double* __restrict__ G, int rows, int64_t ld, const double* __restrict__ P, int ldp,
                                                            const int32_t* __restrict__ cnt, const double* __restrict__ err, int n_dev, int M,
                                                            double* __restrict__ acc, double pk, int first) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const int x = cnt[f];
    const int n_tap = err ? n_dev : 1, half = err ? (n_dev - 1) / 2 : 0;
    double up = 0.0, down = 0.0;
    for (int t = 0; t < n_tap; ++t) {
        const int c = x - half + t;
        double lt = 0.0, eq = 0.0, gt = 0.0, w = 0.0;
        if (c >= 0 && c <= M) {
            w = err ? err[(int64_t)x * n_dev + t] : 1.0;
            for (int i = 0; i < rows; ++i) {
                const double term = G[(int64_t)i * ld + f] * P[(int64_t)i * ldp + c];
                if (i < c) lt += term;
                else if (i > c) gt += term;
                else eq = term;
            }
        }
        const double tot = pk * (w * (lt + eq + gt));
        double* o = acc + (int64_t)t * ld + f;
        *o = first ? tot : *o + tot;
        up += w * lt;
        down += w * gt;
    }
    double* o = acc + (int64_t)n_tap * ld + f;
    o[0] = first ? pk * up : o[0] + pk * up;
    o[ld] = first ? pk * down : o[ld] + pk * down;
}

struct SummaryOut {
    double* mean;
    int32_t *mode, *lo, *hi;
    double *p_inc, *p_dec;
};

// One walk over a node's accumulated posterior: mean, first arg max and the two CDF crossings.  The root's launch also
// produces Z = sum_s acc_root[s] first; every other node is normalised by that Z.
__global__ __launch_bounds__(256) void marginal_summary_kernel(const double* __restrict__ acc, int jmax, int64_t ld, double* __restrict__ Z, int make_z,
                                                               double level, const double* __restrict__ br_inc, const double* __restrict__ br_dec,
                                                               SummaryOut out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double z;
    if (make_z) {
        z = 0.0;
        for (int j = 0; j <= jmax; ++j) z += acc[(int64_t)j * ld + f];
        Z[f] = z;
    } else {
        z = Z[f];
    }
    const double nan = __builtin_nan("");
    if (evidence_failed(z)) {
        out.mean[f] = nan; out.mode[f] = -1; out.lo[f] = -1; out.hi[f] = -1; out.p_inc[f] = nan; out.p_dec[f] = nan;
        return;
    }
    const double tlo = 0.5 * (1.0 - level) * z, thi = (1.0 - 0.5 * (1.0 - level)) * z;
    double cum = 0.0, mean = 0.0, best = -1.0;
    int arg = 0, lo = -1, hi = -1;
    for (int j = 0; j <= jmax; ++j) {
        const double p = acc[(int64_t)j * ld + f];
        if (p > best) { best = p; arg = j; }
        cum += p;
        mean += (double)j * p;
        if (lo < 0 && cum >= tlo) lo = j;
        if (hi < 0 && cum >= thi) hi = j;
    }
    out.mean[f] = mean / z;
    out.mode[f] = arg;
    out.lo[f] = lo < 0 ? jmax : lo;
    out.hi[f] = hi < 0 ? jmax : hi;
    out.p_inc[f] = br_inc ? br_inc[f] / z : nan;
    out.p_dec[f] = br_dec ? br_dec[f] / z : nan;
}

// A leaf's row: the observed count, or with an error model the posterior over its taps (marginal_leaf_kernel's sums)
__global__ __launch_bounds__(256) void marginal_leaf_summary_kernel(const double* __restrict__ acc, const int32_t* __restrict__ cnt, int n_dev, int has_err,
                                                                    int M, int64_t ld, const double* __restrict__ Z, double level, SummaryOut out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const double z = Z[f], nan = __builtin_nan("");
    if (evidence_failed(z)) {
        out.mean[f] = nan; out.mode[f] = -1; out.lo[f] = -1; out.hi[f] = -1; out.p_inc[f] = nan; out.p_dec[f] = nan;
        return;
    }
    const int x = cnt[f];
    const int n_tap = has_err ? n_dev : 1, half = has_err ? (n_dev - 1) / 2 : 0;
    out.p_inc[f] = acc[(int64_t)n_tap * ld + f] / z;
    out.p_dec[f] = acc[(int64_t)(n_tap + 1) * ld + f] / z;
    if (!has_err) {
        out.mean[f] = (double)x; out.mode[f] = x; out.lo[f] = x; out.hi[f] = x;
        return;
    }
    const double tlo = 0.5 * (1.0 - level) * z, thi = (1.0 - 0.5 * (1.0 - level)) * z;
    double cum = 0.0, mean = 0.0, best = -1.0;
    int arg = 0, lo = -1, hi = -1, last = 0;
    for (int t = 0; t < n_tap; ++t) {
        const int c = x - half + t;
        if (c < 0 || c > M) continue;
        const double p = acc[(int64_t)t * ld + f];
        if (p > best) { best = p; arg = c; }
        cum += p;
        mean += (double)c * p;
        if (lo < 0 && cum >= tlo) lo = c;
        if (hi < 0 && cum >= thi) hi = c;
        last = c;
    }
    out.mean[f] = mean / z;
    out.mode[f] = arg;
    out.lo[f] = lo < 0 ? last : lo;
    out.hi[f] = hi < 0 ? last : hi;
}

}  // namespace

int marginal_impl(cafe_ctx* c, const cafe_params* pr, double level, const cafe_marginal_out* out) {
    if (const int rc = check_call_args(c, "cafe_marginal_reconstruct", pr, out)) return rc;
    if (!(level > 0.0 && level < 1.0)) { set_err(c, "cafe_marginal_reconstruct: level must lie in (0, 1)"); return CAFE_ERR_ARGUMENT; }
    if (const int rc = check_model_args(c, "cafe_marginal_reconstruct", pr)) return rc;
    PosteriorCall pc;
    if (const int rc = open_posterior_call(c, pr, &pc)) return rc;
    pc.timer.on = c->profile != 0;
    hipStream_t s = pc.s;
    UpPanels& up = pc.up;
    const int M = c->M, R = c->R, n = c->n_nodes, rows = c->N;      // a panel holds sizes 0..max(M, R)
    const int K = pc.K, nI = pc.nI, n_dev = pc.n_dev, n_tap = n_dev;
    std::vector<int> lidx(n, -1);
    int nL = 0;
    for (int v = 0; v < n; ++v) if (c->leaf_taxon[v] >= 0) lidx[v] = nL++;

    // workspace per column: B, F, O and the accumulation panel of every interior node, G and D, the leaf sums, the branch
    // sums, Z and the summaries
    const size_t dbl_per_col = (size_t)4 * nI * rows + 2 * (size_t)rows + (size_t)nL * (n_tap + 2) + 2 * (size_t)nI + 1 + 3 * (size_t)n;
    const size_t per_col = dbl_per_col * sizeof(double) + (size_t)3 * n * sizeof(int32_t);
    int64_t cols = 0;
    if (const int rc = column_chunk(c, per_col, "cafe_marginal_reconstruct: not enough device memory for the panels of " + std::to_string(nI) + " interior nodes", &cols))
        return rc;
    DevBuf wd, wi;
    if (hipMalloc(&wd.p, dbl_per_col * cols * sizeof(double)) != hipSuccess || hipMalloc(&wi.p, (size_t)3 * n * cols * sizeof(int32_t)) != hipSuccess ||
        alloc_constants(c, kNoPriorLogs, &pc) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "cafe_marginal_reconstruct: cannot allocate the workspace (%lld columns)", (long long)cols);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemsetAsync(wd.p, 0, dbl_per_col * cols * sizeof(double), s));
    const int64_t pstride = (int64_t)rows * cols;
    double* d_O = up.place(wd.p, nI, pstride);
    double* d_A = d_O + (int64_t)nI * pstride;
    double* d_G = d_A + (int64_t)nI * pstride;
    double* d_D = d_G + pstride;
    double* d_leaf = d_D + pstride;                          // [leaf][n_tap + 2][cols]
    double* d_br = d_leaf + (int64_t)nL * (n_tap + 2) * cols;      // [interior node][2][cols]
    double* d_Z = d_br + (int64_t)2 * nI * cols;
    double* d_mean = d_Z + cols;                             // [node][cols]
    double* d_pinc = d_mean + (int64_t)n * cols;
    double* d_pdec = d_pinc + (int64_t)n * cols;
    int32_t* d_mode = static_cast<int32_t*>(wi.p);
    int32_t* d_lo = d_mode + (int64_t)n * cols;
    int32_t* d_hi = d_lo + (int64_t)n * cols;
    if (const int rc = upload_constants(c, pr, &pc)) return rc;

    std::vector<double> h_mean((size_t)n * cols), h_pinc((size_t)n * cols), h_pdec((size_t)n * cols), h_Z(cols);
    std::vector<int32_t> h_mode((size_t)n * cols), h_lo((size_t)n * cols), h_hi((size_t)n * cols);

    const std::vector<Branch> down = branches_down(c);
    for (int64_t f0 = 0; f0 < c->Fp; f0 += cols) {
        const int64_t ld = std::min<int64_t>(cols, c->Fp - f0);
        const unsigned gb = (unsigned)((ld + 255) / 256);
        for (int k = 0; k < K; ++k) {
            const double pk = pc.gamma ? pr->cat_probs[k] : 1.0;
            const int first = k == 0;
            // ---- up: children before parents
            if (const int rc = marginal_up_pass(c, up, k, f0, ld, s, pc.timer)) return rc;
            // ---- root, then parents before children
            CAFE_LAUNCH(c, marginal_root_kernel, dim3(gb, (unsigned)((R + 1 + 15) / 16)), dim3(256), 0, s, up.panel(up.B, c->root), pc.prior, R, ld, up.panel(d_O, c->root),
                        up.panel(d_A, c->root), pk, first);
            for (const Branch& b : down) {
                const int v = b.v, np = b.np;
                GemmParams g;
                if (const int rc = down_branch(c, up, d_O, d_G, b, k, pk, f0, ld, s, &g)) return rc;
                if (c->leaf_taxon[v] >= 0) {
                    CAFE_LAUNCH(c, marginal_leaf_kernel, dim3(gb), dim3(256), 0, s, d_G, np + 1, ld, leaf_matrix(c, v, k), c->pool.ld, leaf_counts(c, v, f0), up.err,
                                n_dev, M, d_leaf + (int64_t)lidx[v] * (n_tap + 2) * cols, pk, first);
                    continue;
                }
                g.out2 = up.panel(d_A, v); g.first = first;
                if (const int rc = launch_gemm<kDown>(c, g, false, s, pc.timer)) return rc;
                for (int m = 1; m <= 2; ++m) {               // the branch split: i < j, then i > j
                    g.mask = m; g.out1 = d_D; g.out2 = nullptr;
                    if (const int rc = launch_gemm<kSplit>(c, g, false, s, pc.timer, 0.5)) return rc;      // about half of the K tiles run
                    CAFE_LAUNCH(c, marginal_colsum_kernel, dim3(gb), dim3(256), 0, s, d_D, M + 1, ld, d_br + ((int64_t)2 * up.bidx[v] + (m - 1)) * cols, pk, first);
                }
            }
        }
        // ---- summaries: the root first (it makes Z)
        for (int pass = 0; pass < 2; ++pass)
            for (int v = 0; v < n; ++v) {
                if ((v == c->root) != (pass == 0)) continue;
                SummaryOut so{d_mean + (int64_t)v * cols, d_mode + (int64_t)v * cols, d_lo + (int64_t)v * cols, d_hi + (int64_t)v * cols,
                              d_pinc + (int64_t)v * cols, d_pdec + (int64_t)v * cols};
                if (c->leaf_taxon[v] >= 0) {
                    CAFE_LAUNCH(c, marginal_leaf_summary_kernel, dim3(gb), dim3(256), 0, s, d_leaf + (int64_t)lidx[v] * (n_tap + 2) * cols, leaf_counts(c, v, f0), n_dev,
                                pc.has_err ? 1 : 0, M, ld, d_Z, level, so);
                } else {
                    const bool is_root = v == c->root;
                    const double* bi = is_root ? nullptr : d_br + (int64_t)2 * up.bidx[v] * cols;
                    CAFE_LAUNCH(c, marginal_summary_kernel, dim3(gb), dim3(256), 0, s, up.panel(d_A, v), is_root ? R : M, ld, d_Z, is_root ? 1 : 0, level, bi,
                                bi ? bi + cols : nullptr, so);
                }
            }
        HIP_TRY(c, hipMemcpyAsync(h_mean.data(), d_mean, sizeof(double) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_pinc.data(), d_pinc, sizeof(double) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_pdec.data(), d_pdec, sizeof(double) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_mode.data(), d_mode, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_lo.data(), d_lo, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_hi.data(), d_hi, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_Z.data(), d_Z, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for_each_family_of_chunk(c, f0, ld, [&](int64_t f, int64_t col) {
            const double z = h_Z[col];
            const bool bad = evidence_failed(z);
            if (out->log_evidence) out->log_evidence[f] = bad ? kNaN : std::log(z);
            if (out->failed) out->failed[f] = bad ? 1 : 0;
            for (int v = 0; v < n; ++v) {
                const size_t src = (size_t)v * cols + col, dst = (size_t)f * n + v;
                if (out->mean) out->mean[dst] = h_mean[src];
                if (out->mode) out->mode[dst] = h_mode[src];
                if (out->lo) out->lo[dst] = h_lo[src];
                if (out->hi) out->hi[dst] = h_hi[src];
                if (out->p_increase) out->p_increase[dst] = h_pinc[src];
                if (out->p_decrease) out->p_decrease[dst] = h_pdec[src];
            }
        });
    }
    close_posterior_call(c, &pc.timer);
    return CAFE_OK;
}

}  // namespace cafe

extern "C" {

int cafe_marginal_reconstruct(cafe_ctx* ctx, const cafe_params* params, double level, const cafe_marginal_out* out) {
    return cafe::guarded_observed(ctx, "cafe_marginal_reconstruct", [&] { return cafe::marginal_impl(ctx, params, level, out); });
}

int cafe_debug_marginal_gemm(cafe_ctx* ctx, double* ms, double* flops) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (ms) *ms = ctx->marginal_gemm_ms;
    if (flops) *flops = ctx->marginal_gemm_flops;
    return CAFE_OK;
}

}
