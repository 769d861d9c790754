// Drawing gene families down a tree on the device, shared by the two Monte-Carlo paths of the library (pvalues.hip,
// simulate.hip): the generator, the uniform, the row CDFs of a row-major matrix pool and the inverse-CDF draw of a child
// size (set_weighted_random_family_size, src/probability.cpp:320-351).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cafe {

// Philox4x32-10 (Salmon et al., SC'11): a counter-based generator, keyed by the caller's seed, so that a draw depends on
// its counter only -- not on launch shape, batching or device.
__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The draw of (family, node) on `stream` (0: the child size, 1: the error-model uniform): counter = (family lo, family hi,
// node, stream), 53 bits of the first two words, in (0,1)
__device__ inline double uniform01(int64_t family, int node, uint32_t stream, uint32_t k0, uint32_t k1) {
    uint32_t r[4];
    philox4x32_10((uint32_t)family, (uint32_t)((uint64_t)family >> 32), (uint32_t)node, stream, k0, k1, r);
    return ((double)(((uint64_t)r[0] << 21) ^ (r[1] >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
}

// The child size of a parent whose row of prefix sums is cdf_row: sizes 0..cols-1 carry the weights (:338-341), the
// first c with cdf_row[c] >= u * cdf_row[cols-1].
// A saturated / degenerate branch has an all-zero row (matrix_cache.cpp:153): the target is 0 and the search returns
// size 0.  The reference draws from std::discrete_distribution over all-zero weights there (probability.cpp:333-344,
// after a uniform draw it then discards) -- outside that distribution's precondition (sum of weights > 0); libstdc++
// returns index 0, so does this, by construction.
__device__ inline int draw_child_size(const double* cdf_row, int cols, double u) {
    const double target = u * cdf_row[cols - 1];
    int lo = 0, hi = cols - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf_row[mid] >= target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Inclusive prefix sums along c = 0..cols-1 of rows 1.. of every matrix of a row-major pool, in place; one wave per row.
// x: matrix (a pool can hold more than 65 535), y: row - 1.  Row 0 is never drawn from: an extinct lineage stays extinct.
static __global__ __launch_bounds__(64) void row_cdf_kernel(double* __restrict__ base, int64_t stride, int ld, int cols) {
    const int row = blockIdx.y + 1, lane = threadIdx.x;
    double* r = base + (int64_t)blockIdx.x * stride + (int64_t)row * ld;
    double carry = 0.0;
    for (int c0 = 0; c0 < cols; c0 += 64) {
        const int c = c0 + lane;
        double v = c < cols ? r[c] : 0.0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double up = __shfl_up(v, d);
            if (lane >= d) v += up;
        }
        v += carry;
        if (c < cols) r[c] = v;
        carry = __shfl(v, 63);
    }
}

// rows 1..rows-1 of n_slots matrices
inline hipError_t launch_row_cdf(double* base, int64_t stride, int ld, int n_slots, int rows, int cols, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(row_cdf_kernel, dim3(n_slots, rows - 1), dim3(64), 0, stream, base, stride, ld, cols);
    return hipGetLastError();
}

}  // namespace cafe
