// Per-branch scores for a rate-shift scan, and their information.
//
// cafe_branch_scores is cafe_score_gradient's walk (gradient.hip, gradient_walk) with a score panel: for the branch above v
// the walk forms G_v^T (dP_v / d theta) B_v per category and free rate and adds it, weighted p_k, into one sum per lambda
// index.  With a panel the dot and leaf kernels add the same sum once more, weighted p_k m_k lambda_q (or mu_q) -- a factor c_v
// on the rate of that branch alone moves lambda_q m_k by lambda_q m_k d log c_v -- into the branch's own row: one row per
// (branch, rate), the categories already mixed.  The panel S [P][Fp] holds those rows and the global scores of every
// distinct family over all column batches; after the last batch
//     gram = S diag(w) S^T,   total = S w,      w = the multiplicity of each distinct family,
// on the fp64 MFMA.  The Gram matrix: a wave owns one 16 x 16 tile of the lower triangle over one slab of kGramSlab columns
// (slabs are cut on the global column index), stages 16 rows x 64 columns of both operands in LDS and issues sixteen
// v_mfma_f64_16x16x4_f64 per stage; a second kernel adds the slabs' partial tiles in slab order and writes the tile and its
// mirror image (of a diagonal tile: its lower half and the mirror of that).  No atomics: the bits depend on (P, columns,
// kGramSlab) only, and gram is exactly symmetric.  total is a row sum in the same manner: per (row, slab) a wave's strided
// sums folded by a fixed tree, then the slabs in order.
#include <cmath>
#include <vector>

#include "sum_product.h"

namespace cafe {

namespace {

constexpr int kGramSlab = 2048;         // columns per partial tile
constexpr int kGC = 64;                 // columns per stage
constexpr int kLdG = kGC + 4;           // LDS row stride: the 16 rows of a fragment load start 8 banks apart

// tile t of the lower triangle, rows first: (0,0) (1,0) (1,1) (2,0) ...
__device__ inline void gram_tile(int t, int* bi, int* bj) {
    int i = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    while (i * (i + 1) / 2 > t) --i;
    *bi = i;
    *bj = t - i * (i + 1) / 2;
}

// part[slab][tile][16][16] = S_bi diag(w) S_bj^T over the slab's columns.  A = S_bi w (fragment: row = lane & 15, k = lane >> 4),
// B = S_bj^T (k = lane >> 4, column = lane & 15), D: row = (lane >> 4) + 4 * register, column = lane & 15.  Rows >= P, columns
// >= n and columns of weight 0 are staged as zeros whatever S holds there.
__global__ __launch_bounds__(64) void weighted_gram_tile_kernel(const double* __restrict__ S, int64_t lds, const double* __restrict__ w, int P, int64_t n,
                                                                int n_tiles, double* __restrict__ part) {
    __shared__ double As[16 * kLdG], Bs[16 * kLdG];
    const int lane = threadIdx.x, l15 = lane & 15, l4 = lane >> 4;
    const int t = blockIdx.x, slab = blockIdx.y;
    int bi, bj;
    gram_tile(t, &bi, &bj);
    const int64_t c_begin = (int64_t)slab * kGramSlab, c_end = min(n, c_begin + kGramSlab);
    typedef double d4 __attribute__((ext_vector_type(4)));
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
    for (int64_t c0 = c_begin; c0 < c_end; c0 += kGC) {
        const int64_t col = c0 + lane;
        const double wv = col < c_end ? w[col] : 0.0;
        const bool live = wv != 0.0;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ra = 16 * bi + r, rb = 16 * bj + r;
            As[r * kLdG + lane] = (live && ra < P) ? S[(int64_t)ra * lds + col] * wv : 0.0;
            Bs[r * kLdG + lane] = (live && rb < P) ? S[(int64_t)rb * lds + col] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kGC / 4; ++s)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[l15 * kLdG + 4 * s + l4], Bs[l15 * kLdG + 4 * s + l4], acc, 0, 0, 0);
    }
    double* o = part + ((int64_t)slab * n_tiles + t) * 256;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[(l4 + 4 * q) * 16 + l15] = acc[q];
}

// tpart[slab][row] = sum over the slab's columns of w S[row]: lane l takes the columns l, l + 64, ... in order, the 64 sums
// fold by halves
__global__ __launch_bounds__(64) void weighted_gram_rowsum_kernel(const double* __restrict__ S, int64_t lds, const double* __restrict__ w, int P, int64_t n,
                                                                  double* __restrict__ tpart) {
    __shared__ double red[64];
    const int lane = threadIdx.x, row = blockIdx.x, slab = blockIdx.y;
    const int64_t c_begin = (int64_t)slab * kGramSlab, c_end = min(n, c_begin + kGramSlab);
    double s = 0.0;
    for (int64_t col = c_begin + lane; col < c_end; col += 64) {
        const double wv = w[col];
        if (wv != 0.0) s += S[(int64_t)row * lds + col] * wv;
    }
    red[lane] = s;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (lane < off) red[lane] += red[lane + off];
        __syncthreads();
    }
    if (lane == 0) tpart[(int64_t)slab * P + row] = red[0];
}

// The slabs in order: entry e < n_tiles * 256 is one element of one tile -> gram (and its mirror image); the P entries behind
// them are the rows of total.  gram / total may be nullptr.
__global__ __launch_bounds__(256) void weighted_gram_reduce_kernel(const double* __restrict__ part, const double* __restrict__ tpart, int n_slabs, int n_tiles, int P,
                                                                   double* __restrict__ gram, double* __restrict__ total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_el = (int64_t)n_tiles * 256;
    if (e < n_el) {
        if (!gram) return;
        const int t = (int)(e >> 8), r = (int)(e >> 4) & 15, cc = (int)e & 15;
        int bi, bj;
        gram_tile(t, &bi, &bj);
        const int i = 16 * bi + r, j = 16 * bj + cc;
        if (i >= P || j >= P || j > i) return;               // a diagonal tile: its lower half
        double s = 0.0;
        for (int k = 0; k < n_slabs; ++k) s += part[(int64_t)k * n_el + e];
        gram[(int64_t)i * P + j] = s;
        gram[(int64_t)j * P + i] = s;
        return;
    }
    const int64_t row = e - n_el;
    if (row >= P || !total) return;
    double s = 0.0;
    for (int k = 0; k < n_slabs; ++k) s += tpart[(int64_t)k * P + row];
    total[row] = s;
}

// One batch's rows of the panel divided by Z as the finish kernel divides the sums; a failed column: zeros (NaN times a
// zero weight would be NaN)
__global__ __launch_bounds__(256) void score_panel_finish_kernel(const double* __restrict__ Z, int64_t ld, int64_t stride, int n_rows, double* __restrict__ rows) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const double z = Z[f];
    const bool bad = evidence_failed(z);
    for (int j = 0; j < n_rows; ++j) {
        double* o = rows + (int64_t)j * stride + f;
        *o = bad ? 0.0 : *o / z;
    }
}

// gram [P][P] and total [P] (device pointers, either may be nullptr) of the device panel S [P][lds], columns 0..n-1
// ms, flops (may be nullptr): the HIP-event time of the launches and the flops of the tiles' MFMAs
hipError_t gram_on_device(hipStream_t s, int P, int64_t n, const double* S, int64_t lds, const double* w, double* gram, double* total, double* ms = nullptr,
                          double* flops = nullptr) {
    const int nb = (P + 15) / 16, n_tiles = nb * (nb + 1) / 2;
    const int n_slabs = (int)((n + kGramSlab - 1) / kGramSlab);
    if (n_slabs > 65535) return hipErrorInvalidValue;
    DevBuf part, tpart;
    hipError_t e;
    if ((e = hipMalloc(&part.p, sizeof(double) * 256 * (size_t)n_tiles * n_slabs)) != hipSuccess) return e;
    if ((e = hipMalloc(&tpart.p, sizeof(double) * (size_t)P * n_slabs)) != hipSuccess) return e;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (ms && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) ms = nullptr;
    (void)hipGetLastError();
    if (ms) (void)hipEventRecord(ev[0], s);
    if (gram) hipLaunchKernelGGL(weighted_gram_tile_kernel, dim3((unsigned)n_tiles, (unsigned)n_slabs), dim3(64), 0, s, S, lds, w, P, n, n_tiles, static_cast<double*>(part.p));
    if (total) hipLaunchKernelGGL(weighted_gram_rowsum_kernel, dim3((unsigned)P, (unsigned)n_slabs), dim3(64), 0, s, S, lds, w, P, n, static_cast<double*>(tpart.p));
    const int64_t n_el = (int64_t)n_tiles * 256 + P;
    hipLaunchKernelGGL(weighted_gram_reduce_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, s, static_cast<const double*>(part.p),
                       static_cast<const double*>(tpart.p), n_slabs, n_tiles, P, gram, total);
    e = hipGetLastError();
    if (ms) (void)hipEventRecord(ev[1], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);        // the partial tiles are freed on return
    if (ms) {
        float t = 0.f;
        *ms = e == hipSuccess && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess ? t : 0.0;
    }
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
    if (flops) *flops = gram ? 2.0 * 256.0 * n_tiles * (double)n : 0.0;
    return e;
}

}  // namespace

// ------------------------------------------------------------------------------------------------- the panel of the walk
int score_panel_open(cafe_ctx* c, const char* entry, int n_par, int n_glob, ScorePanel* sp) {
    sp->n_par = n_par;
    sp->n_glob = n_glob;
    sp->n_branch = c->n_nodes - 1;
    sp->P = n_par * sp->n_branch + n_glob;
    sp->Fp = c->Fp;
    c->gram_ms = c->gram_flops = 0.0;
    sp->slot.assign(c->n_nodes, -1);
    for (int v = 0, i = 0; v < c->n_nodes; ++v) if (v != c->root) sp->slot[v] = i++;
    sp->col_failed.assign((size_t)c->Fp, 1);                 // padding columns stay failed: they carry no family
    const size_t bytes = sizeof(double) * (size_t)sp->P * (size_t)sp->Fp;
    HIP_TRY(c, hipSetDevice(c->device));
    if (hipMalloc(&sp->S.p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "%s: not enough device memory for the score panel (%d scores x %lld columns, %.1f MB)", entry, sp->P, (long long)sp->Fp, bytes / 1e6);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemsetAsync(sp->S.p, 0, bytes, c->stream));
    return CAFE_OK;
}

int score_panel_batch(cafe_ctx* c, hipStream_t s, ScorePanel* sp, int64_t f0, int64_t ld, int64_t cols, const double* d_Z, const double* h_Z,
                      const double* h_glob) {
    const cafe_branch_scores_out* out = sp->out;
    const int n_rows = sp->n_par * sp->n_branch, n = c->n_nodes;
    double* rows = sp->base() + f0;
    CAFE_LAUNCH(c, score_panel_finish_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, s, d_Z, ld, sp->Fp, n_rows, rows);
    for (int64_t col = 0; col < ld; ++col) sp->col_failed[(size_t)(f0 + col)] = evidence_failed(h_Z[col]) ? 1 : 0;
    // the global scores: the numbers the caller gets, so that gram is the Gram matrix of the rows it returns
    std::vector<double> glob((size_t)sp->n_glob * ld);
    for (int g = 0; g < sp->n_glob; ++g)
        for (int64_t col = 0; col < ld; ++col) glob[(size_t)g * ld + col] = sp->col_failed[(size_t)(f0 + col)] ? 0.0 : h_glob[(size_t)g * cols + col];
    HIP_TRY(c, hipMemcpy2DAsync(rows + (int64_t)n_rows * sp->Fp, sizeof(double) * sp->Fp, glob.data(), sizeof(double) * ld, sizeof(double) * ld, sp->n_glob,
                                hipMemcpyHostToDevice, s));
    std::vector<double> h;
    if (out->rate || out->birth || out->death) {
        h.resize((size_t)n_rows * ld);
        HIP_TRY(c, hipMemcpy2DAsync(h.data(), sizeof(double) * ld, rows, sizeof(double) * sp->Fp, sizeof(double) * ld, n_rows, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (h.empty()) return CAFE_OK;
    for_each_family_of_chunk(c, f0, ld, [&](int64_t f, int64_t col) {
        const bool bad = sp->col_failed[(size_t)(f0 + col)] != 0;
        for (int v = 0; v < n; ++v) {
            const int i = sp->slot[v];
            const bool nan = bad || i < 0;
            const double b = nan ? kNaN : h[(size_t)i * ld + col];
            const double d = nan || sp->n_par < 2 ? kNaN : h[(size_t)(sp->n_branch + i) * ld + col];
            if (out->rate) out->rate[f * n + v] = sp->n_par < 2 ? b : b + d;
            if (out->birth) out->birth[f * n + v] = b;
            if (out->death) out->death[f * n + v] = d;
        }
    });
    return CAFE_OK;
}

int score_panel_close(cafe_ctx* c, hipStream_t s, ScorePanel* sp) {
    const cafe_branch_scores_out* out = sp->out;
    std::vector<double> w((size_t)sp->Fp, 0.0);
    int64_t used = 0;
    for (int64_t u = 0; u < c->F_uniq; ++u)
        if (!sp->col_failed[(size_t)u]) { w[(size_t)u] = c->weights[(size_t)u]; used += (int64_t)c->weights[(size_t)u]; }
    if (out->n_used) *out->n_used = used;
    if (!out->gram && !out->total) return CAFE_OK;
    const size_t P = (size_t)sp->P;
    DevBuf dw, dg, dt;
    if (hipMalloc(&dw.p, sizeof(double) * w.size()) != hipSuccess || (out->gram && hipMalloc(&dg.p, sizeof(double) * P * P) != hipSuccess) ||
        (out->total && hipMalloc(&dt.p, sizeof(double) * P) != hipSuccess)) {
        (void)hipGetLastError();
        set_err(c, "cafe_branch_scores: not enough device memory for the Gram matrix of %d scores", sp->P);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemcpyAsync(dw.p, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, s));
    const hipError_t e = gram_on_device(s, sp->P, sp->Fp, sp->base(), sp->Fp, static_cast<const double*>(dw.p), static_cast<double*>(dg.p), static_cast<double*>(dt.p),
                                        c->profile ? &c->gram_ms : nullptr, &c->gram_flops);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        set_err(c, "cafe_branch_scores: not enough device memory for the partial tiles of the Gram matrix of %d scores", sp->P);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, e);
    if (out->gram) HIP_TRY(c, hipMemcpy(out->gram, dg.p, sizeof(double) * P * P, hipMemcpyDeviceToHost));
    if (out->total) HIP_TRY(c, hipMemcpy(out->total, dt.p, sizeof(double) * P, hipMemcpyDeviceToHost));
    return CAFE_OK;
}

static int branch_scores_dim(const cafe_ctx* c, const cafe_params* pr) {
    const int n_par = c->mus.empty() ? 1 : 2;
    return n_par * (c->n_nodes - 1) + c->n_lambdas * n_par + (pr->model == CAFE_MODEL_GAMMA ? pr->n_categories : 0);
}

int branch_scores_impl(cafe_ctx* c, const cafe_params* pr, int32_t root_rule, const cafe_branch_scores_out* out) {
    if (const int rc = check_call_args(c, "cafe_branch_scores", pr, out)) return rc;
    if ((out->birth || out->death) && c->mus.empty()) {
        set_err(c, "cafe_branch_scores: birth and death need death rates (cafe_set_death_rates)");
        return CAFE_ERR_STATE;
    }
    cafe_gradient_out g{};
    g.family_lnl = out->family_lnl; g.d_lambda = out->d_lambda; g.d_mu = out->d_mu; g.d_multiplier = out->d_multiplier; g.failed = out->failed;
    ScorePanel sp;
    sp.out = out;
    return gradient_walk(c, "cafe_branch_scores", pr, root_rule, &g, &sp);
}

}  // namespace cafe

extern "C" {

int cafe_branch_scores(cafe_ctx* ctx, const cafe_params* params, int32_t root_rule, const cafe_branch_scores_out* out) {
    return cafe::guarded_observed(ctx, "cafe_branch_scores", [&] { return cafe::branch_scores_impl(ctx, params, root_rule, out); });
}

int cafe_branch_scores_dim(const cafe_ctx* ctx, const cafe_params* params, int32_t* P) {
    if (!ctx || !params || !P) return CAFE_ERR_ARGUMENT;
    *P = cafe::branch_scores_dim(ctx, params);
    return CAFE_OK;
}

int cafe_debug_gram(cafe_ctx* ctx, double* ms, double* flops) {
    if (!ctx || !ms || !flops) return CAFE_ERR_ARGUMENT;
    *ms = ctx->gram_ms;
    *flops = ctx->gram_flops;
    return CAFE_OK;
}

int cafe_weighted_gram(int32_t device, int32_t p, int64_t n, const double* S, const double* w, double* gram, double* total) {
    if (p < 1 || n < 1 || !S || !w || (!gram && !total)) return CAFE_ERR_ARGUMENT;
    if (hipSetDevice(device) != hipSuccess) return CAFE_ERR_DEVICE;
    cafe::DevBuf dS, dw, dg, dt;
    const size_t P = (size_t)p;
    if (hipMalloc(&dS.p, sizeof(double) * P * n) != hipSuccess || hipMalloc(&dw.p, sizeof(double) * n) != hipSuccess ||
        (gram && hipMalloc(&dg.p, sizeof(double) * P * P) != hipSuccess) || (total && hipMalloc(&dt.p, sizeof(double) * P) != hipSuccess)) {
        (void)hipGetLastError();
        return CAFE_ERR_MEMORY;
    }
    if (hipMemcpy(dS.p, S, sizeof(double) * P * n, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dw.p, w, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess)
        return CAFE_ERR_DEVICE;
    const hipError_t e = cafe::gram_on_device(nullptr, p, n, static_cast<const double*>(dS.p), n, static_cast<const double*>(dw.p), static_cast<double*>(dg.p),
                                              static_cast<double*>(dt.p));
    if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? CAFE_ERR_MEMORY : e == hipErrorInvalidValue ? CAFE_ERR_ARGUMENT : CAFE_ERR_DEVICE; }
    if (gram && hipMemcpy(gram, dg.p, sizeof(double) * P * P, hipMemcpyDeviceToHost) != hipSuccess) return CAFE_ERR_DEVICE;
    if (total && hipMemcpy(total, dt.p, sizeof(double) * P, hipMemcpyDeviceToHost) != hipSuccess) return CAFE_ERR_DEVICE;
    return CAFE_OK;
}

}
