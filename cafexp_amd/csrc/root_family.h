// Internal: what K4 makes of ONE family's root column(s), and the deterministic final sum -- the arithmetic shared by the
// kernels of a single call (leaf_reduce.hip: root_reduce_kernel, root_reduce_sum_kernel, partial_sum_kernel) and by the
// kernels of a batch of parameter vectors (root_reduce_batch.hip), so that a point of a batch gets the bits cafe_score gives
// it.  The shape is the one root_sum.h describes: kRedFam families x kRedSeg row segments per 256-thread workgroup, thread
// (family, segment) walks the rows j = segment, segment + kRedSeg, ... of its family's column.  Every function here is
// entered by all 256 threads (they meet at barriers); the value it returns is complete in the threads with seg == 0.
#pragma once
#include "root_sum.h"

namespace cafe {

// Maxima do not depend on the order they are combined in; the category sum is only tested against zero (all terms are
// non-negative).  NaN follows the reference's scan (std::max_element / the `>` scan of gamma_core.cpp:158): a NaN at j = 0 is
// returned, a NaN elsewhere never wins a comparison.
constexpr int kRedFam = 16, kRedSeg = 16;
static_assert(kRedFam == kSumFam && kRedSeg == kSumSeg, "both root rules share one workgroup shape");
__device__ inline double combine_max(double* sh, int fam, int seg, double v) {
    sh[seg * kRedFam + fam] = v;
    __syncthreads();
    double best = sh[fam];
    if (seg == 0)
        for (int s2 = 1; s2 < kRedSeg; ++s2) { const double p = sh[s2 * kRedFam + fam]; if (p > best) best = p; }
    __syncthreads();
    return best;
}
__device__ inline double combine_sum(double* sh, int fam, int seg, double v) {
    sh[seg * kRedFam + fam] = v;
    __syncthreads();
    double t = 0.0;
    if (seg == 0)
        for (int s2 = 0; s2 < kRedSeg; ++s2) t += sh[s2 * kRedFam + fam];
    __syncthreads();
    return t;
}

// Base model, CAFE_ROOT_MAX: lnL_f = max_j( log L_j + log prior_j ), first maximum like std::max_element (base_model.cpp:94-101)
__device__ inline double family_base_max(const double* col, int32_t ld, int R, const double* log_prior, bool live, double* sh, int fam, int seg) {
    double best = -__builtin_huge_val();
    if (live)
        for (int j = seg; j < R; j += kRedSeg) {
            const double full = log(col[(int64_t)j * ld]) + log_prior[j];
            if (j == 0 || full > best) best = full;
        }
    return combine_max(sh, fam, seg, best);
}

// Gamma model, CAFE_ROOT_MAX: lik_f = sum_k p_k max_j(L^k_j prior_j) over the K categories that start at `col`, kstride apart
// (gamma_core.cpp:144-166, 201-225).  cat_out: the family's [K] category likelihoods, or nullptr.  *fail: a category's root
// vector summed to exactly 0.
__device__ inline double family_gamma_max(const double* col, int64_t kstride, int32_t ld, int R, int K, const double* prior, const double* cat_probs,
                                          bool live, double* sh, int fam, int seg, double* cat_out, int* fail) {
    const double ninf = -__builtin_huge_val();
    double lik = 0.0;
    int bad = 0;
    for (int k = 0; k < K; ++k) {
        const double* ck = col + (int64_t)k * kstride;
        double sum = 0.0, best = ninf;
        if (live)
            for (int j = seg; j < R; j += kRedSeg) {
                const double L = ck[(int64_t)j * ld];
                sum += L;
                const double full = L * prior[j];
                if (j == 0 || full > best) best = full;
            }
        sum = combine_sum(sh, fam, seg, sum);
        best = combine_max(sh, fam, seg, best);
        if (live && seg == 0) {
            if (sum == 0.0) bad = 1;                       // "saturation", gamma_core.cpp:152
            const double cl = best * cat_probs[k];          // gamma_core.cpp:162
            if (cat_out) cat_out[k] = cl;
            lik += cl;                                      // gamma_core.cpp:207
        }
    }
    *fail = bad;
    return lik;
}

// Gamma model, CAFE_ROOT_SUM: p_k sum_j L_j prior_j per category in the linear domain (column_sum, root_sum.h)
__device__ inline double family_gamma_sum(const double* col, int64_t kstride, int32_t ld, int R, int K, const double* prior, const double* cat_probs,
                                          bool live, double* sh, int fam, int seg, double* cat_out, int* fail) {
    double lik = 0.0;
    int bad = 0;
    for (int k = 0; k < K; ++k) {
        double plain;
        const double s = column_sum(col + (int64_t)k * kstride, ld, R, prior, live, sh, fam, seg, &plain);
        if (live && seg == 0) {
            if (plain == 0.0) bad = 1;                     // "saturation", gamma_core.cpp:152
            const double cl = s * cat_probs[k];
            if (cat_out) cat_out[k] = cl;
            lik += cl;
        }
    }
    *fail = bad;
    return lik;
}

// Deterministic two-stage sum: fixed block partials, then one block folds them in index order.
__device__ inline double block_sum(double v, double* sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    __syncthreads();
    return t;
}

// Block `block` of `n_blocks` of the final sum: its 256-element strides of sum_f w_f fam_out[f] and of the weight of the failed
// families into scratch[2 block ..]; the block that finishes last folds the partials, in index order whichever block that
// is, into out[0..1] (and out2[0..1] when not null: host memory the device can write).  scratch: [2 * n_blocks] partials, then
// one unsigned counter (zero between calls: the folding block resets it).  sh: 4 doubles, last: one flag, both in LDS.
__device__ inline void final_sum_block(const double* __restrict__ fam_out, const double* __restrict__ w, const int32_t* __restrict__ failed, int64_t n,
                                       double* scratch, double* out, double* out2, unsigned block, unsigned n_blocks, double* sh, bool* last) {
    double s = 0.0, bad = 0.0;
    for (int64_t i = (int64_t)block * 256 + threadIdx.x; i < n; i += (int64_t)n_blocks * 256) {
        s += w[i] * fam_out[i];
        bad += failed[i] ? w[i] : 0.0;
    }
    const double ts = block_sum(s, sh);
    const double tb = block_sum(bad, sh);
    unsigned* counter = reinterpret_cast<unsigned*>(scratch + 2 * n_blocks);
    if (threadIdx.x == 0) {
        scratch[2 * block] = ts;
        scratch[2 * block + 1] = tb;
        __threadfence();                                     // the partials are visible before the ticket is taken
        *last = atomicAdd(counter, 1u) == n_blocks - 1;
    }
    __syncthreads();
    if (!*last || threadIdx.x != 0) return;
    __threadfence();
    double fs = 0.0, fb = 0.0;
    const volatile double* sc = scratch;                     // (written by other blocks of this launch)
    for (unsigned i = 0; i < n_blocks; ++i) {
        fs += sc[2 * i];
        fb += sc[2 * i + 1];
    }
    out[0] = fs;
    out[1] = fb;
    if (out2) { out2[0] = fs; out2[1] = fb; }
    *counter = 0u;
}
// blocks of the final sum over n values with room for n_scratch partials
inline int final_sum_blocks(int64_t n, int n_scratch) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > n_scratch) blocks = n_scratch;
    return blocks < 1 ? 1 : blocks;
}

// K4 and the final sum for a batch of G parameter vectors that went through the prune as G * K categories of one call
// (root_reduce_batch.hip): point g owns the categories g K .. g K + K - 1 of the root panel and row g of cat_probs.
struct ReduceBatchArgs {
    const double* root;             // root panel [G * K][i][family]
    int64_t panel_kstride;
    int32_t ld, R;
    int32_t K;                      // categories per point (1: base model)
    int32_t G;                      // points
    int32_t model;                  // 0 base, 1 gamma
    int32_t root_sum;               // CAFE_ROOT_SUM
    const double* prior;            // [R]
    const double* log_prior;        // [R]
    const double* cat_probs;        // [G][K]
    int64_t f0, nf;                 // the chunk: first family, real families
    int64_t F;                      // families: the stride between the points' rows of fam_out / failed
    double* fam_out;                // [G][F]
    int32_t* failed;                // [G][F]
};
hipError_t launch_root_reduce_batch(const ReduceBatchArgs& a, hipStream_t stream);
// per point g: sum_f w_f fam_out[g][f] and the weight of its failed families -> out[2 g ..] and out_host[2 g ..], with
// launch_final_sum's block partition; scratch: [G][2 * n_scratch + 1] doubles, zero before the first call
hipError_t launch_final_sum_batch(const double* fam_out, const double* weights, const int32_t* failed, int64_t n, int G, double* scratch, int n_scratch,
                                  double* out, double* out_host, hipStream_t stream);

}  // namespace cafe
