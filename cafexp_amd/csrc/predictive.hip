// Leave-one-out predictive check of every leaf count: the distribution of species l's count given the counts of every other
// species of the family.
//
// The model is cafe_marginal_reconstruct's (marginal.hip): the call's lambdas, categories, prior and error model, the context's
// death rates when set, the root weight of CAFE_ROOT_SUM.  For family f, leaf l with parent p and category k:
//     G_l^k[i] = O_p^k[i] prod_{siblings w of l} F_w^k[i]       what down_branch forms (parent = root: i = 1..R, row 0 is 0)
//     O_l^k[c] = sum_{i = 0..np} P_l^k[i][c] G_l^k[i]           c = 0..M
//     u[c]     = sum_k p_k O_l^k[c]                             (p_k = 1, K = 1 for the base model)
//     w[y]     = u[y]                                           without an error model
//              = sum_t err[y][t] u[y - half + t]                with one; taps outside [0, M] dropped: leaf_factor's rule with x = y
//     W        = sum_{y = 0..M} w[y]
// w[x_l] = Z_f, the evidence, and nothing on the right depends on x_l: w / W is the predictive distribution of the leaf's count
// over 0..M (the matrices are cut there, as everywhere in this model).  Per cell (f, l), x the observed count:
//     p_below = sum_{y < x} w / W      p_obs = w[x] / W      p_above = sum_{y > x} w / W      (W: the three added in that order)
//     mean = sum y w / T0,  var = sum y^2 w / T0 - mean^2 clamped at 0,  T0 = sum_y w in the order of y
// The tails are sums, never complements.  mean and sd take their moments about 0 and their own total T0, not about x and not
// W: the rounding of a moment about x, and of a total split at x, depends on x, and the mean and sd of a cell are promised
// not to (a count the user does not trust must not leak into its own imputation, not even in the last bit).  The price is the
// cancellation factor 1 + mean^2 / var where 1 + (mean - x)^2 / var was possible; the factors y and y^2 are exact.
// W zero or not finite: NaN in all five.  All six sums are linear in O, so the categories add into them with weight p_k and no
// panel per leaf is kept: one scratch panel takes every GEMM's output.
//
// The GEMM is sum_product.hip's geometry with other addressing: the leaf matrices are row-major, and read transposed -- for one
// parent size i the 64 child sizes c of a row tile are consecutive in memory -- they are the coalesced A read of that file's up
// pass; row i = 0 is stored and takes part, so neither X nor the output is offset.
#include <cmath>
#include <string>
#include <vector>

#include "sum_product.h"

namespace cafe {

namespace {

// ---------------------------------------------------------------------------------------------------------------- GEMM
// out[c][f] = sum_{i = 0..nk-1} P[i ldp + c] G[i][f], c = 0..nr-1.  Block tile 64 rows x 128 families, K step 16; wave w owns the
// 32 families 32w.. over all 64 rows: 4 x 2 accumulator tiles of v_mfma_f64_16x16x4_f64 (fragment layouts: sum_product.hip).
// Both tiles are staged in LDS k-major with a 16-double pad; the next K step's global loads are in flight while the current
// one is multiplied.  Every load is guarded by nr / nk: nothing depends on padding rows.
constexpr int kMT = 64, kNT = 128, kKT = 16;
constexpr int kLdA = kMT + 16, kLdX = kNT + 16;

struct PredictiveGemm {
    const double* P;        // row-major matrix of the leaf branch
    int ldp;
    const double* G;        // rows = sizes 0..nk-1 of the leaf's parent
    int64_t ld;             // columns of the batch's panels (a multiple of 128)
    int nr, nk;             // child sizes 0..nr-1; parent sizes 0..nk-1
    double* out;            // [nr][ld]
};

__global__ __launch_bounds__(256) void predictive_gemm_kernel(const PredictiveGemm a) {
    __shared__ __attribute__((aligned(16))) double As[kKT * kLdA];
    __shared__ __attribute__((aligned(16))) double Xs[kKT * kLdX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int r0 = blockIdx.y * kMT;
    const int64_t c0 = (int64_t)blockIdx.x * kNT;
    const int nr = a.nr, nk = a.nk, ldp = a.ldp;
    const int64_t ld = a.ld;
    typedef double d4 __attribute__((ext_vector_type(4)));
    d4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
    double ra[4];
    double2 rx[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + lane, k = k0 + wave + 4 * u;  // A[r][k] = P[k][r]: 64 consecutive child sizes per parent size
            ra[u] = (r < nr && k < nk) ? a.P[(int64_t)k * ldp + r] : 0.0;
            rx[u] = k < nk ? *reinterpret_cast<const double2*>(a.G + (int64_t)k * ld + c0 + 2 * lane) : make_double2(0.0, 0.0);
        }
    };
    load(0);
    for (int k0 = 0; k0 < nk; k0 += kKT) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            As[(wave + 4 * u) * kLdA + lane] = ra[u];
            *reinterpret_cast<double2*>(&Xs[(wave + 4 * u) * kLdX + 2 * lane]) = rx[u];
        }
        __syncthreads();
        if (k0 + kKT < nk) load(k0 + kKT);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            double af[4], bf[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = As[(4 * s4 + l4) * kLdA + 16 * i + l15];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Xs[(4 * s4 + l4) * kLdX + 32 * wave + 16 * j + l15];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 16 * i + l4 + 4 * q;
                if (r >= nr) continue;
                a.out[(int64_t)r * ld + c0 + 32 * wave + 16 * j + l15] = acc[i][j][q];
            }
}

// ---------------------------------------------------------------------------------------------------------------- sums
// One thread per column walks y = 0..M over the GEMM's panel U, forms w[y] from its taps on the fly and adds
// p_k {sum_{y < x} w, w[x], sum_{y > x} w, sum w, sum y w, sum y^2 w} into the six sums of the (leaf, column): acc[j][f], j-th row
// `stride` doubles on.  The first category stores, the others add.  A missing cell (x = CAFE_COUNT_MISSING) indexes nothing
// here: every y lies above it, the three totals t0, t1, t2 are what they are for any x, and its w[x] slot carries NaN, by
// which predictive_finish_kernel knows the cell and turns its tails into NaN.
constexpr int kSums = 6;
__global__ __launch_bounds__(256) void predictive_sums_kernel(const double* __restrict__ U, int M, int64_t ld, const int32_t* __restrict__ cnt,
                                                              const double* __restrict__ err, int n_dev, double pk, int first,
                                                              double* __restrict__ acc, int64_t stride) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const int x = cnt[f];
    const int half = (n_dev - 1) / 2;
    double below = 0.0, obs = 0.0, above = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int y = 0; y <= M; ++y) {
        double w;
        if (err == nullptr) {
            w = U[(int64_t)y * ld + f];
        } else {
            w = 0.0;
            for (int t = 0; t < n_dev; ++t) {
                const int c = y - half + t;
                if (c < 0 || c > M) continue;
                w += U[(int64_t)c * ld + f] * err[(int64_t)y * n_dev + t];
            }
        }
        if (y < x) below += w;
        else if (y > x) above += w;
        else obs = w;
        t0 += w;
        t1 += (double)y * w;
        t2 += (double)(y * y) * w;
    }
    if (count_is_missing(x)) obs = __builtin_nan("");      // no observation: the mark predictive_finish_kernel reads (a NaN w[x] comes with a NaN t0)
    const double s[kSums] = {below, obs, above, t0, t1, t2};
#pragma unroll
    for (int j = 0; j < kSums; ++j) {
        double* o = acc + (int64_t)j * stride + f;
        *o = first ? pk * s[j] : *o + pk * s[j];
    }
}

// Per column (blockIdx.x) and leaf (blockIdx.y): the five outputs over the first five of the leaf's six sums, in the order
// mean, sd, p_below, p_obs, p_above; NaN in all five where W or the total is zero or not finite.  A missing cell (w[x] NaN beside
// a total that is not: predictive_sums_kernel) has no observation: its three tail outputs are NaN, its mean and sd -- which read
// t0, t1, t2 only -- are the model's prediction of the count from the family's other species.
__global__ __launch_bounds__(256) void predictive_finish_kernel(double* __restrict__ acc, int64_t ld, int64_t stride) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double* a = acc + (int64_t)blockIdx.y * kSums * stride + f;
    const double below = a[0], obs = a[stride], above = a[2 * stride], t0 = a[3 * stride], t1 = a[4 * stride], t2 = a[5 * stride];
    const double nan = __builtin_nan("");
    const bool missing = obs != obs && t0 == t0;
    const double W = below + obs + above;
    const bool bad = (!missing && evidence_failed(W)) || evidence_failed(t0);
    const double mean = t1 / t0;
    const double var = fmax(t2 / t0 - mean * mean, 0.0);
    a[0] = bad ? nan : mean;
    a[stride] = bad ? nan : sqrt(var);
    a[2 * stride] = bad ? nan : below / W;
    a[3 * stride] = bad ? nan : obs / W;
    a[4 * stride] = bad ? nan : above / W;
}

}  // namespace

int leaf_predictive_impl(cafe_ctx* c, const cafe_params* pr, const cafe_leaf_predictive_out* out) {
    if (const int rc = check_call_args(c, "cafe_leaf_predictive", pr, out)) return rc;
    if (const int rc = check_model_args(c, "cafe_leaf_predictive", pr)) return rc;
    PosteriorCall pc;
    if (const int rc = open_posterior_call(c, pr, &pc)) return rc;
    pc.timer.on = c->profile != 0;
    hipStream_t s = pc.s;
    UpPanels& up = pc.up;
    const int M = c->M, R = c->R, rows = c->N, n = c->n_nodes, K = pc.K, nI = pc.nI, nT = c->n_taxa;
    std::vector<int> lidx(n, -1);
    int nL = 0;
    for (int v = 0; v < n; ++v) if (c->leaf_taxon[v] >= 0) lidx[v] = nL++;

    // workspace per column: B, F and O of every interior node; G, the panel that takes the down GEMM's second output and the
    // panel of the leaf GEMM; Z_k, the six sums per leaf, Z and its logarithm
    const size_t dbl_per_col = (size_t)3 * nI * rows + 3 * (size_t)rows + K + (size_t)kSums * nL + 2;
    int64_t cols = 0;
    if (const int rc = column_chunk(c, dbl_per_col * sizeof(double),
                                    "cafe_leaf_predictive: not enough device memory for the panels of " + std::to_string(nI) + " interior nodes", &cols))
        return rc;
    DevBuf wd;
    if (hipMalloc(&wd.p, dbl_per_col * cols * sizeof(double)) != hipSuccess || alloc_constants(c, kNoPriorLogs, &pc) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "cafe_leaf_predictive: cannot allocate the workspace (%lld columns)", (long long)cols);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemsetAsync(wd.p, 0, dbl_per_col * cols * sizeof(double), s));
    const int64_t pstride = (int64_t)rows * cols;
    double* d_O = up.place(wd.p, nI, pstride);
    double* d_G = d_O + (int64_t)nI * pstride;
    double* d_S = d_G + pstride;                             // the down GEMM's posterior product: not read
    double* d_U = d_S + pstride;                             // O_l of one leaf and category
    double* d_zk = d_U + pstride;                            // [K][cols]
    double* d_acc = d_zk + (int64_t)K * cols;                // [leaf][6][cols]
    double* d_Z = d_acc + (int64_t)kSums * nL * cols;
    double* d_lnl = d_Z + cols;
    if (const int rc = upload_constants(c, pr, &pc)) return rc;
    std::vector<double> h_acc((size_t)kSums * nL * cols), h_Z(cols), h_lnl(cols);
    double* const dst[5] = {out->mean, out->sd, out->p_below, out->p_obs, out->p_above};

    const std::vector<Branch> down = branches_down(c);
    for (int64_t f0 = 0; f0 < c->Fp; f0 += cols) {
        const int64_t ld = std::min<int64_t>(cols, c->Fp - f0);
        const unsigned gb = (unsigned)((ld + 255) / 256);
        for (int k = 0; k < K; ++k) {
            const double pk = pc.gamma ? pr->cat_probs[k] : 1.0;
            if (const int rc = marginal_up_pass(c, up, k, f0, ld, s, pc.timer)) return rc;
            if (const int rc = launch_root_weights(c, s, up.panel(up.B, c->root), pc.prior, nullptr, R, ld, up.panel(d_O, c->root),
                                                   d_zk + (int64_t)k * cols, nullptr, CAFE_ROOT_SUM, 0))
                return rc;
            for (const Branch& b : down) {
                GemmParams g;
                if (const int rc = down_branch(c, up, d_O, d_G, b, k, pk, f0, ld, s, &g)) return rc;
                if (c->leaf_taxon[b.v] < 0) {
                    g.out2 = d_S; g.first = 1;               // O_v is all that is wanted
                    if (const int rc = launch_gemm<kDown>(c, g, false, s, pc.timer)) return rc;
                    continue;
                }
                PredictiveGemm pg{};
                pg.P = leaf_matrix(c, b.v, k); pg.ldp = c->pool.ld; pg.G = d_G; pg.ld = ld; pg.nr = M + 1; pg.nk = b.np + 1; pg.out = d_U;
                pc.timer.mark(s);
                CAFE_LAUNCH(c, predictive_gemm_kernel, dim3((unsigned)(ld / kNT), (unsigned)((pg.nr + kMT - 1) / kMT)), dim3(256), 0, s, pg);
                pc.timer.mark(s);
                pc.timer.flops += 2.0 * pg.nr * pg.nk * (double)ld;
                CAFE_LAUNCH(c, predictive_sums_kernel, dim3(gb), dim3(256), 0, s, (const double*)d_U, M, ld, leaf_counts(c, b.v, f0), up.err, up.n_dev, pk,
                            k == 0 ? 1 : 0, d_acc + (int64_t)lidx[b.v] * kSums * cols, cols);
            }
        }
        if (const int rc = launch_finish_sums(c, s, d_zk, pc.probs, K, ld, cols, nullptr, d_acc, 0, d_Z, d_lnl)) return rc;
        CAFE_LAUNCH(c, predictive_finish_kernel, dim3(gb, (unsigned)nL), dim3(256), 0, s, d_acc, ld, cols);
        HIP_TRY(c, hipMemcpyAsync(h_acc.data(), d_acc, sizeof(double) * (size_t)kSums * nL * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_Z.data(), d_Z, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_lnl.data(), d_lnl, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for_each_family_of_chunk(c, f0, ld, [&](int64_t f, int64_t col) {
            const bool bad = evidence_failed(h_Z[col]);
            if (out->log_evidence) out->log_evidence[f] = bad ? kNaN : h_lnl[col];
            if (out->failed) out->failed[f] = bad ? 1 : 0;
            for (int v = 0; v < n; ++v) {
                if (lidx[v] < 0) continue;
                for (int j = 0; j < 5; ++j)
                    if (dst[j]) dst[j][f * nT + c->leaf_taxon[v]] = h_acc[((size_t)lidx[v] * kSums + j) * cols + col];
            }
        });
    }
    close_posterior_call(c, &pc.timer);
    return CAFE_OK;
}

}  // namespace cafe

extern "C" {

int cafe_leaf_predictive(cafe_ctx* ctx, const cafe_params* params, const cafe_leaf_predictive_out* out) {
    return cafe::guarded(ctx, "cafe_leaf_predictive", [&] { return cafe::leaf_predictive_impl(ctx, params, out); });
}

}
