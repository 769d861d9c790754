// cafe_root_posterior: P(root size | data) of every family on the scorer's own prune, and its sum over the table -- the E step
// of a maximum-likelihood update of the root distribution (prior_new[j] = total[j] / n_used).
//
// The call is a scorer call (enqueue, cafe_score.hip: K1, the schedule with subtree sharing and zero extents, K2 / K3) whose
// root panel is read by two kernels where K4 and the final sum stand, per column chunk:
//   column kernel  root_reduce_kernel's shape (16 families x 16 row segments per workgroup, whole 128-byte lines per wave
//                  instruction).  Per distinct column: Z = sum_k p_k sum_j prior_j L^k_j with the sum rule's reductions
//                  (root_sum.h: the bits cafe_score gives under CAFE_ROOT_SUM), log Z, the posterior mean and first arg max of
//                  the root size, the category posteriors p_k Z_k / Z, and the column's scale w / Z (w its multiplicity; 0
//                  for a failed or a padding column).
//   row kernel     one workgroup per root row j: total[j] += sum_f scale_f sum_k p_k L^k_j[f].  A panel row is contiguous
//                  along the columns, so this streams: a wave takes a 128-column tile (16 bytes per lane), sums it by a
//                  fixed tree and parks the tile's sum in LDS; one thread folds the tiles in tile order onto the running
//                  total.  Chunks are multiples of 128 columns, so total has the same bits however workspace_limit cuts the
//                  columns.  The prior's factor is applied once, on the host, behind the last chunk.
// No atomics, no scratch.  Bound: HBM / L2 traffic of the root panel, read three times (the second and third from L2).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "cafe_call.h"
#include "root_sum.h"
#include "sum_product.h"

namespace cafe {

namespace {

constexpr int kRowTiles = 512;                  // tile sums parked in LDS between two folds (4 KB)

__global__ __launch_bounds__(256) void root_posterior_column_kernel(const ReduceArgs a, const RootPosteriorArgs p) {
    __shared__ double sh[kSumFam * kSumSeg];
    __shared__ int sh_arg[kSumFam * kSumSeg];
    const int fam = threadIdx.x % kSumFam, seg = threadIdx.x / kSumFam;
    const int64_t fl = (int64_t)blockIdx.x * kSumFam + fam;       // the grid covers the chunk's ld columns, padding included
    const bool live = fl < a.nf;                                  // (every thread reaches the barriers)
    const int64_t f = a.f0 + fl;
    const double* col = a.root + fl;
    // ---- Z = sum_k p_k Z_k (cat_probs is 1.0 under the base model)
    double Z = 0.0;
    for (int k = 0; k < a.K; ++k) {
        double plain;
        const double zk = column_sum(col + (int64_t)k * a.panel_kstride, a.ld, a.R, a.prior, live, sh, fam, seg, &plain);
        const double pz = zk * a.cat_probs[k];
        Z += pz;
        if (p.cat_post && live && seg == 0) p.cat_post[f * a.K + k] = pz;
    }
    const double log_z = a.model == 0 ? column_log_sum(col, a.ld, a.R, a.log_prior, live, sh, fam, seg) : log(Z);
    // ---- mean and first arg max of prior_j sum_k p_k L^k_j
    double m1 = 0.0, best = -__builtin_huge_val();
    int arg = 0x7fffffff;
    if (live)
        for (int j = seg; j < a.R; j += kSumSeg) {
            double mix = 0.0;
            for (int k = 0; k < a.K; ++k) mix += a.cat_probs[k] * col[(int64_t)k * a.panel_kstride + (int64_t)j * a.ld];
            const double pj = a.prior[j] * mix;
            m1 += (double)(j + 1) * pj;
            if (pj > best) { best = pj; arg = j; }
        }
    m1 = seg_sum(sh, fam, seg, m1);
    sh[seg * kSumFam + fam] = best;
    sh_arg[seg * kSumFam + fam] = arg;
    __syncthreads();
    if (seg != 0) return;
    if (!live) { p.scale[f] = 0.0; return; }
    for (int s2 = 1; s2 < kSumSeg; ++s2) {              // the segments interleave the rows: on equal masses the smaller row
        const double b2 = sh[s2 * kSumFam + fam];
        const int a2 = sh_arg[s2 * kSumFam + fam];
        if (b2 > best || (b2 == best && a2 < arg)) { best = b2; arg = a2; }
    }
    const bool bad = evidence_failed(Z);
    const double nan = __builtin_nan("");
    p.Z[f] = Z;
    p.log_z[f] = bad ? nan : log_z;
    p.mean[f] = bad ? nan : m1 / Z;
    p.mode[f] = bad || arg == 0x7fffffff ? -1 : arg + 1;
    if (p.cat_post)
        for (int k = 0; k < a.K; ++k) p.cat_post[f * a.K + k] = bad ? nan : p.cat_post[f * a.K + k] / Z;
    p.scale[f] = bad ? 0.0 : p.weights[f] / Z;
}

__global__ __launch_bounds__(256) void root_posterior_row_kernel(const ReduceArgs a, const RootPosteriorArgs p) {
    __shared__ double tile_sum[kRowTiles];
    const int j = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n_tiles = a.ld / kBN;
    const double* __restrict__ row = a.root + (int64_t)j * a.ld;
    const double* __restrict__ scale = p.scale + a.f0;
    double run = threadIdx.x == 0 ? p.row_total[j] : 0.0;
    for (int t0 = 0; t0 < n_tiles; t0 += kRowTiles) {
        const int nb = min(kRowTiles, n_tiles - t0);
        for (int t = w; t < nb; t += 4) {
            const int64_t c = (int64_t)(t0 + t) * kBN + 2 * lane;
            const double2 sc = *reinterpret_cast<const double2*>(scale + c);
            double mx = 0.0, my = 0.0;
            for (int k = 0; k < a.K; ++k) {
                const double2 L = *reinterpret_cast<const double2*>(row + (int64_t)k * a.panel_kstride + c);
                mx += a.cat_probs[k] * L.x;
                my += a.cat_probs[k] * L.y;
            }
            // (a failed or a padding column has scale 0 and whatever in the panel: it adds an exact 0)
            double v = (sc.x != 0.0 ? sc.x * mx : 0.0) + (sc.y != 0.0 ? sc.y * my : 0.0);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
            if (lane == 0) tile_sum[t] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int t = 0; t < nb; ++t) run += tile_sum[t];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.row_total[j] = run;
}

inline size_t even(size_t n) { return (n + 1) / 2 * 2; }

}  // namespace

hipError_t launch_root_posterior(const ReduceArgs& a, const RootPosteriorArgs& p, hipStream_t stream) {
    if (a.ld <= 0 || a.ld % kBN != 0 || a.f0 % kBN != 0 || a.R < 1 || (a.model != 0 && a.model != 1)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(root_posterior_column_kernel, dim3((unsigned)(a.ld / kSumFam)), dim3(256), 0, stream, a, p);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(root_posterior_row_kernel, dim3((unsigned)a.R), dim3(256), 0, stream, a, p);
    return hipGetLastError();
}

int root_posterior_impl(cafe_ctx* c, const cafe_params* pr, const cafe_root_posterior_out* out) {
    const char* const who = "cafe_root_posterior";
    if (const int rc = check_call_args(c, who, pr, out)) return rc;
    if (const int rc = check_model_args(c, who, pr)) return rc;
    const bool gamma = pr->model == CAFE_MODEL_GAMMA;
    if (out->category_posterior && !gamma) { set_err(c, "%s: category_posterior belongs to the gamma model", who); return CAFE_ERR_ARGUMENT; }
    if (!c->device_ready || !c->d_counts) { set_err(c, "%s: the context holds no family table", who); return CAFE_ERR_STATE; }
    const int K = gamma ? pr->n_categories : 1, R = c->R;
    const size_t Fu = (size_t)c->F_uniq, Fp = (size_t)c->Fp;
    HIP_TRY(c, hipSetDevice(c->device));

    // ---- the call's device arrays: one allocation, every double array on a 16-byte boundary
    const size_t o_logz = even(Fu), o_mean = o_logz + even(Fu), o_total = o_mean + even(Fu), o_scale = o_total + even((size_t)R),
                 o_cat = o_scale + even(Fp), o_mode = o_cat + (out->category_posterior ? even(Fu * K) : 0), n_doubles = o_mode + even(Fu) / 2 + 1;
    DevBuf buf;
    if (hipMalloc(&buf.p, sizeof(double) * n_doubles) != hipSuccess) {
        (void)hipGetLastError();
        buf.p = nullptr;
        set_err(c, "%s: cannot allocate the workspace (%zu bytes)", who, sizeof(double) * n_doubles);
        return CAFE_ERR_MEMORY;
    }
    double* base = static_cast<double*>(buf.p);
    RootPosteriorArgs ra{};
    ra.weights = c->d_weights;
    ra.Z = base; ra.log_z = base + o_logz; ra.mean = base + o_mean; ra.row_total = base + o_total; ra.scale = base + o_scale;
    ra.cat_post = out->category_posterior ? base + o_cat : nullptr;
    ra.mode = reinterpret_cast<int32_t*>(base + o_mode);
    HIP_TRY(c, hipMemsetAsync(ra.row_total, 0, sizeof(double) * (size_t)R, c->stream));

    // ---- one scorer call with the two kernels in K4's place
    if (const int rc = enqueue(c, pr, c->d_result, c->stream, false, &ra)) { fail_after_enqueue(c, c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // (a device error from here on: cafe_root_posterior below)
    close_posterior_call(c, nullptr);                   // the matrices stay readable; cafe_family_results is not meaningful
    collect_stats(c);

    // ---- read back, per distinct column; spread over the table
    std::vector<double> Z(Fu), tmp(Fu * (size_t)std::max(1, K)), total((size_t)R);
    HIP_TRY(c, hipMemcpy(Z.data(), ra.Z, sizeof(double) * Fu, hipMemcpyDeviceToHost));
    std::vector<int32_t> bad(Fu);
    double used = 0.0;
    bool any_nan = false;
    for (size_t u = 0; u < Fu; ++u) {
        bad[u] = evidence_failed(Z[u]) ? 1 : 0;
        any_nan = any_nan || std::isnan(Z[u]);
        if (!bad[u]) used += c->weights[u];
    }
    if (any_nan) c->panels_dirty = true;                // NaNs may now sit in the panels (see record_call)
    if (out->failed) spread_unique(c, bad.data(), out->failed);
    if (out->n_used) *out->n_used = (int64_t)std::llround(used);
    if (out->log_evidence) {
        HIP_TRY(c, hipMemcpy(tmp.data(), ra.log_z, sizeof(double) * Fu, hipMemcpyDeviceToHost));
        spread_unique(c, tmp.data(), out->log_evidence);
    }
    if (out->mean) {
        HIP_TRY(c, hipMemcpy(tmp.data(), ra.mean, sizeof(double) * Fu, hipMemcpyDeviceToHost));
        spread_unique(c, tmp.data(), out->mean);
    }
    if (out->category_posterior) {
        HIP_TRY(c, hipMemcpy(tmp.data(), ra.cat_post, sizeof(double) * Fu * K, hipMemcpyDeviceToHost));
        spread_unique(c, tmp.data(), out->category_posterior, K);
    }
    if (out->mode) {
        std::vector<int32_t> mode(Fu);
        HIP_TRY(c, hipMemcpy(mode.data(), ra.mode, sizeof(int32_t) * Fu, hipMemcpyDeviceToHost));
        spread_unique(c, mode.data(), out->mode);
    }
    if (out->total) {
        HIP_TRY(c, hipMemcpy(total.data(), ra.row_total, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost));
        for (int j = 0; j < R; ++j) out->total[j] = (double)pr->prior[j] * total[(size_t)j];     // compute() returns float
    }
    return CAFE_OK;
}

}  // namespace cafe

int cafe_root_posterior(cafe_ctx* ctx, const cafe_params* params, const cafe_root_posterior_out* out) {
    const int rc = cafe::guarded(ctx, "cafe_root_posterior", [&] { return cafe::root_posterior_impl(ctx, params, out); });
    if (rc == CAFE_ERR_DEVICE) cafe::fail_after_enqueue(ctx, ctx->stream);
    return rc;
}
