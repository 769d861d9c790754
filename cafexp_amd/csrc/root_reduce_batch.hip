// K4 and the final sum of cafe_score_batch: G parameter vectors went through K1, the prepass, K2 and K3 as G * K categories of
// one call; behind the root panel every point needs its own reduction.  Two launches whatever G is -- where a call is the sum
// of its kernels' latencies, G launches of the single-call kernels would give the batch's gain away:
//   root_reduce_batch_kernel   grid (families / 16, G): root_reduce_kernel's / root_reduce_sum_kernel's workgroup for point
//                              blockIdx.y, on that point's K categories of the panel -> fam_out[g][f], failed[g][f]
//   final_sum_batch_kernel     grid (blocks, G): partial_sum_kernel's blocks for point blockIdx.y, on that point's scratch
//                              region and ticket -> {sum lnL, rejects}[g], also written straight to pinned host memory
// The arithmetic is root_family.h's and root_sum.h's, the code the single-call kernels run: same loops, same order, same
// block partition.  Bound: latency (one pass over a panel of R rows x families x G K categories; the sums are tiny).
#include "root_family.h"

namespace cafe {

__global__ __launch_bounds__(256) void root_reduce_batch_kernel(const ReduceBatchArgs a) {
    __shared__ double sh[kRedFam * kRedSeg];
    const int fam = threadIdx.x % kRedFam, seg = threadIdx.x / kRedFam;
    const int64_t fl = (int64_t)blockIdx.x * kRedFam + fam;
    const bool live = fl < a.nf;                            // (every thread reaches the barriers)
    const int g = blockIdx.y;
    const double* col = a.root + (int64_t)g * a.K * a.panel_kstride + fl;
    const int64_t o = (int64_t)g * a.F + a.f0 + fl;
    if (a.model == 0) {
        const double v = a.root_sum ? column_log_sum(col, a.ld, a.R, a.log_prior, live, sh, fam, seg)
                                    : family_base_max(col, a.ld, a.R, a.log_prior, live, sh, fam, seg);
        if (live && seg == 0) { a.fam_out[o] = v; a.failed[o] = 0; }
        return;
    }
    const double* cat_probs = a.cat_probs + (int64_t)g * a.K;
    int fail = 0;
    const double lik = a.root_sum ? family_gamma_sum(col, a.panel_kstride, a.ld, a.R, a.K, a.prior, cat_probs, live, sh, fam, seg, nullptr, &fail)
                                  : family_gamma_max(col, a.panel_kstride, a.ld, a.R, a.K, a.prior, cat_probs, live, sh, fam, seg, nullptr, &fail);
    if (live && seg == 0) {
        a.fam_out[o] = log(lik);
        a.failed[o] = fail;
    }
}

hipError_t launch_root_reduce_batch(const ReduceBatchArgs& a, hipStream_t stream) {
    if (a.nf <= 0) return hipSuccess;
    if ((a.model != 0 && a.model != 1) || a.G < 1 || a.G > 65535 || a.K < 1 || (a.model == 0 && a.K != 1) || a.f0 + a.nf > a.F) return hipErrorInvalidValue;
    dim3 grid((unsigned)((a.nf + kRedFam - 1) / kRedFam), (unsigned)a.G), block(256);
    (void)hipGetLastError();
    hipLaunchKernelGGL(root_reduce_batch_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

// scratch_stride: doubles between the points' scratch regions (partials of every block, then the ticket)
__global__ __launch_bounds__(256) void final_sum_batch_kernel(const double* __restrict__ fam_out, const double* __restrict__ w,
                                                              const int32_t* __restrict__ failed, int64_t n, double* scratch, int64_t scratch_stride,
                                                              double* out, double* out2) {
    __shared__ double sh[4];
    __shared__ bool last;
    const int g = blockIdx.y;
    final_sum_block(fam_out + (int64_t)g * n, w, failed + (int64_t)g * n, n, scratch + (int64_t)g * scratch_stride, out + 2 * g,
                    out2 ? out2 + 2 * g : nullptr, blockIdx.x, gridDim.x, sh, &last);
}

hipError_t launch_final_sum_batch(const double* fam_out, const double* weights, const int32_t* failed, int64_t n, int G, double* scratch, int n_scratch,
                                  double* out, double* out_host, hipStream_t stream) {
    if (G < 1 || G > 65535) return hipErrorInvalidValue;
    const int blocks = final_sum_blocks(n, n_scratch);
    (void)hipGetLastError();
    hipLaunchKernelGGL(final_sum_batch_kernel, dim3(blocks, G), dim3(256), 0, stream, fam_out, weights, failed, n, scratch,
                       (int64_t)(2 * n_scratch + 1), out, out_host);
    return hipGetLastError();
}

}  // namespace cafe
