// The per-family branch kernel (family_lambda.hip has the reasoning), one body for both rate models: the kernel, its argument
// block and its launcher are templates on the slot type.  family_lambda.hip instantiates SlotParam (cafe_score_per_family),
// family_lambda_lm.hip SlotParamLM (cafe_score_per_family_lm); the host frame of the entries is family_frame.h's.  The slot
// decides the row step's constants (bd_row.h) through slot_tail / slot_q and nothing else.  Only the ROW-MAJOR recurrence is
// involved -- row 0 is e_0, the factor is sum_c P[s][c] v[c] of the process itself -- so the exchange identity of the k-major
// build (bd_matrix.hip) plays no part here.
#pragma once

#include "bd_row.h"
#include "cafe_kernels.h"

namespace cafe {

// The parked dot product (family_lambda.hip has the reasoning)
constexpr int kPartRows = 16;        // rows whose lane partials are parked before they are summed
constexpr int kPartLd = 65;          // doubles per parked row: 64 lanes + 1, so that the transposed read spreads over the banks

template <class Slot>
struct FamLamArgs {
    const int32_t* nodes;            // the nodes of this level: one unit of work per branch above them
    const int32_t* child_off;        // [n_nodes + 1] children of a node: child_idx[child_off[u] .. child_off[u + 1])
    const int32_t* child_idx;
    const int32_t* taxon;            // [n_nodes] row of `counts` for a leaf, -1 for interior nodes
    const int32_t* n_rows;           // [n_nodes] factor rows s = 0..n_rows-1: M + 1, or R + 1 under the root
    const Slot* slots;               // [batch][n_nodes] the branch's parameters under the family's lambdas (and mus)
    const int64_t* col;              // [batch] the family's column in `counts`
    const int32_t* counts;           // [taxon][counts_ld]
    int64_t counts_ld;
    const double* err;               // [(M+1)][n_dev] or nullptr
    int32_t n_dev, M, ld, n_nodes;
    double* factors;                 // [batch][n_nodes][ld]
};

template <class Slot, int E>
__global__ __launch_bounds__(64) void family_lambda_kernel(const FamLamArgs<Slot> a) {
    __shared__ double part[kPartRows * kPartLd];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int u = a.nodes[blockIdx.y];
    const Slot sp = a.slots[b * a.n_nodes + u];
    double* __restrict__ fac_b = a.factors + b * a.n_nodes * a.ld;
    double* __restrict__ out = fac_b + (int64_t)u * a.ld;
    const int c0 = lane * E;                           // owned columns c0 .. c0+E-1 of the current row
    const int n_rows = a.n_rows[u];

    double v[E];                                       // the child's likelihoods of sizes c0 .. c0+E-1 (0 past M)
    const int tx = a.taxon[u];
    if (tx >= 0) {                                     // probability.cpp:179-199
        const int x = a.counts[(int64_t)tx * a.counts_ld + a.col[b]];
        if (count_is_missing(x)) {                     // a missing cell: the factor is exactly 1.0 for every parent size (cafe_kernels.h),
            for (int r = lane; r < n_rows; r += 64) out[r] = leaf_factor_or_one(x, 0.0);       // no row of the recurrence is run
            return;                                    // (block-uniform: the block is one (family, branch))
        }
        if (a.err) {
            const int lo = x - (a.n_dev - 1) / 2;      // taps outside [0, M] are dropped
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int c = c0 + i, t = c - lo;
                v[i] = (t >= 0 && t < a.n_dev && c <= a.M) ? a.err[(int64_t)x * a.n_dev + t] : 0.0;
            }
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = (c0 + i == x) ? 1.0 : 0.0;
        }
    } else {                                           // probability.cpp:211-218: the product of the children's factors
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (c0 + i <= a.M) ? 1.0 : 0.0;
        for (int k = a.child_off[u]; k < a.child_off[u + 1]; ++k) {
            const double* __restrict__ f = fac_b + (int64_t)a.child_idx[k] * a.ld;
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (c0 + i <= a.M) v[i] *= f[c0 + i];
        }
    }

    if (sp.zero) {                                     // saturated / degenerate (slot_param, slot_param_lm): rows s >= 1 are 0, row 0 = e_0
        for (int r = lane; r < n_rows; r += 64) out[r] = r == 0 ? v[0] : 0.0;
        return;
    }

    BdRowConsts<E, Slot::two_rates> rc;                // row-major: the process itself, outer = alpha, tail ratio = beta (or alpha)
    rc.init(sp.alpha, slot_tail(sp), slot_q(sp), lane);
    double p[E];                                       // P[row][c0 + i]; columns past the matrix hold values in [0,1] that meet v = 0
#pragma unroll
    for (int i = 0; i < E; ++i) p[i] = (c0 + i == 0) ? 1.0 : 0.0;

    for (int r = 0; r < n_rows; ++r) {
        if (r > 0) bd_row_step<E, false>(rc, nullptr, 0.0, lane, p);
        double d = p[0] * v[0];
#pragma unroll
        for (int i = 1; i < E; ++i) d = fma(p[i], v[i], d);
        part[(r & (kPartRows - 1)) * kPartLd + lane] = d;
        if ((r & (kPartRows - 1)) == kPartRows - 1 || r == n_rows - 1) {
            __syncthreads();                           // one wave per block: orders the LDS writes before the transposed reads
            const int j = lane & 15, quarter = lane >> 4;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += part[j * kPartLd + quarter * 16 + k];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            const int row = (r & ~(kPartRows - 1)) + j;
            if (lane < 16 && row <= r) out[row] = s;
            __syncthreads();                           // the block is read before the next rows overwrite it
        }
    }
}

// one level of branches for `batch` listed families: grid (batch, n_level_nodes), one wave each; n = matrix order
template <class Slot>
hipError_t launch_family_lambda(const FamLamArgs<Slot>& a, int n, int64_t batch, int n_level_nodes, hipStream_t stream) {
    if (batch <= 0 || n_level_nodes <= 0) return hipSuccess;
    if (n > bd_matrix_max_order() || n > a.ld || batch > 0x7fffffff || n_level_nodes > 65535) return hipErrorInvalidValue;
    dim3 grid((unsigned)batch, (unsigned)n_level_nodes), block(64);
    return for_lane_width(n, [&](auto e) {
        (void)hipGetLastError();
        hipLaunchKernelGGL((family_lambda_kernel<Slot, decltype(e)::value>), grid, block, 0, stream, a);
        return hipGetLastError();
    });
}
// each instantiated in the translation unit of its slot type, and nowhere else
extern template hipError_t launch_family_lambda<SlotParam>(const FamLamArgs<SlotParam>&, int, int64_t, int, hipStream_t);
extern template hipError_t launch_family_lambda<SlotParamLM>(const FamLamArgs<SlotParamLM>&, int, int64_t, int, hipStream_t);

}  // namespace cafe
