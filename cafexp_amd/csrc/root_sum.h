// Internal: the sum rule's reductions of a root column (cafe_set_root_rule), shared by the scorer's sum-rule K4
// (leaf_reduce.hip) and the per-column kernel of cafe_root_posterior (root_posterior.hip), so that both give the same bits.
// The shape is root_reduce_kernel's: kRedFam families x kRedSeg row segments per 256-thread workgroup, thread (family,
// segment) walks the rows j = segment, segment + kRedSeg, ... of its family's column (a wave instruction reads kRedFam
// consecutive families of 64 / kRedFam rows: whole 128-byte lines); a thread adds its rows in ascending order, the segments
// are combined in LDS in segment order.  A value therefore depends on the column and R only.
#pragma once
#include "cafe_kernels.h"

namespace cafe {

constexpr int kSumFam = 16, kSumSeg = 16;

// sum over the segments of a family in segment order, to every thread of the family (every thread reaches the barriers)
__device__ inline double seg_sum(double* sh, int fam, int seg, double v) {
    sh[seg * kSumFam + fam] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int s2 = 0; s2 < kSumSeg; ++s2) t += sh[s2 * kSumFam + fam];
    __syncthreads();
    return t;
}
// ... and the maximum (a NaN never wins a comparison: it shows in the sum that follows)
__device__ inline double seg_max(double* sh, int fam, int seg, double v) {
    sh[seg * kSumFam + fam] = v;
    __syncthreads();
    double best = sh[fam];
#pragma unroll
    for (int s2 = 1; s2 < kSumSeg; ++s2) { const double p = sh[s2 * kSumFam + fam]; if (p > best) best = p; }
    __syncthreads();
    return best;
}

// log sum_j L_j prior_j = m + log sum_j exp(t_j - m), t_j = log L_j + log_prior[j], m = max_j t_j.  Finite where the product
// underflows; all t_j = -inf: -inf (a term of -inf adds an exact 0, so that m = -inf never meets inf - inf); a NaN term: NaN.
__device__ inline double column_log_sum(const double* col, int64_t ld, int R, const double* __restrict__ log_prior, bool live, double* sh,
                                        int fam, int seg) {
    const double ninf = -__builtin_huge_val();
    double m = ninf;
    if (live)
        for (int j = seg; j < R; j += kSumSeg) {
            const double t = log(col[(int64_t)j * ld]) + log_prior[j];
            if (t > m) m = t;
        }
    m = seg_max(sh, fam, seg, m);
    double s = 0.0;
    if (live)
        for (int j = seg; j < R; j += kSumSeg) {
            const double t = log(col[(int64_t)j * ld]) + log_prior[j];
            s += t == ninf ? 0.0 : exp(t - m);
        }
    s = seg_sum(sh, fam, seg, s);
    return m + log(s);
}

// sum_j L_j prior_j in the linear domain; *plain = sum_j L_j (the reference's saturation test reads it, gamma_core.cpp:152)
__device__ inline double column_sum(const double* col, int64_t ld, int R, const double* __restrict__ prior, bool live, double* sh, int fam,
                                    int seg, double* plain) {
    double s = 0.0, p = 0.0;
    if (live)
        for (int j = seg; j < R; j += kSumSeg) {
            const double L = col[(int64_t)j * ld];
            p += L;
            s += L * prior[j];
        }
    *plain = seg_sum(sh, fam, seg, p);
    return seg_sum(sh, fam, seg, s);
}

// K4 under CAFE_ROOT_SUM (leaf_reduce.hip): ReduceArgs::model 0 base, 1 gamma
hipError_t launch_root_reduce_sum(const ReduceArgs& a, hipStream_t stream);

// cafe_root_posterior's two kernels behind a chunk's root panel (root_posterior.hip).  Per distinct column (global index):
// Z, log Z, mean, mode, cat_post [column][K] and the column's scale w / Z (0: failed or padding; [Fp], every column of the
// chunk is written).  row_total[R]: the running sum over the columns so far of scale * sum_k p_k L^k_j, before the prior.
struct RootPosteriorArgs {
    const double* weights;          // [F_uniq] multiplicity of a distinct column
    double* Z;
    double* log_z;
    double* mean;
    int32_t* mode;
    double* cat_post;               // nullptr: not asked for
    double* scale;
    double* row_total;
};
hipError_t launch_root_posterior(const ReduceArgs& a, const RootPosteriorArgs& p, hipStream_t stream);

}  // namespace cafe
