// cafe_score_per_family_lm: the per-family branch kernel under SEPARATE birth and death rates -- the two-rate twin of
// family_lambda_kernel (family_lambda.hip), which stays what cafe_score_per_family launches.
//
// The structure is family_lambda.hip's: ONE 64-lane wave per (listed family, branch); the child's likelihood vector v in
// registers; the row recurrence, and after every row step factor[s] = sum_c P[s][c] v[c]; the lane partials parked in LDS and
// summed transposed every 16 rows; one launch per tree level; family_root_kernel closes a family.  What differs:
//   row step   bd_row_step_lm on BdRowConstsLM (bd_row_lm.h): the scan and the h recurrence run on beta, the outer FMA on alpha
//   slot       SlotParamLM from slot_param_lm(quantize(lambda), quantize(mu), quantize(t)); `zero` follows that function's rule
// Only the ROW-MAJOR recurrence is involved -- row 0 is e_0, the factor is sum_c P[s][c] v[c] of the process itself -- so the
// exchange identity of the k-major build (bd_matrix_lm.hip) plays no part here.  With alpha == beta every operand of every
// instruction is family_lambda_kernel's, and so is every bit of the result.
#include <hip/hip_runtime.h>

#include "bd_row_lm.h"
#include "family_lambda_lm.h"

namespace cafe {

namespace {

// MIRROR of family_lambda_kernel (family_lambda.hip): the two bodies differ in the slot type, rc.init and the row step only.
// Until both are one template on the row-step type (with K1 and its twin), a fix to one is a fix to both.
template <int E>
__global__ __launch_bounds__(64) void family_lambda_lm_kernel(const FamLamArgsLM a) {
    __shared__ double part[kPartRows * kPartLd];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int u = a.nodes[blockIdx.y];
    const SlotParamLM sp = a.slots[b * a.n_nodes + u];
    double* __restrict__ fac_b = a.factors + b * a.n_nodes * a.ld;
    double* __restrict__ out = fac_b + (int64_t)u * a.ld;
    const int c0 = lane * E;                           // owned columns c0 .. c0+E-1 of the current row
    const int n_rows = a.n_rows[u];

    double v[E];                                       // the child's likelihoods of sizes c0 .. c0+E-1 (0 past M)
    const int tx = a.taxon[u];
    if (tx >= 0) {                                     // probability.cpp:179-199
        const int x = a.counts[(int64_t)tx * a.counts_ld + a.col[b]];
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

    if (sp.zero) {                                     // saturated / degenerate (slot_param_lm): rows s >= 1 are 0, row 0 = e_0
        for (int r = lane; r < n_rows; r += 64) out[r] = r == 0 ? v[0] : 0.0;
        return;
    }

    BdRowConstsLM<E> rc;                               // row-major: the process itself, outer = alpha, tail ratio = beta
    rc.init(sp.alpha, sp.beta, sp.q, lane);
    double p[E];                                       // P[row][c0 + i]; columns past the matrix hold values in [0,1] that meet v = 0
#pragma unroll
    for (int i = 0; i < E; ++i) p[i] = (c0 + i == 0) ? 1.0 : 0.0;

    for (int r = 0; r < n_rows; ++r) {
        if (r > 0) bd_row_step_lm<E, false>(rc, nullptr, 0.0, lane, p);
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

}  // namespace

hipError_t launch_family_lambda_lm(const FamLamArgsLM& a, int n, int64_t batch, int n_level_nodes, hipStream_t stream) {
    if (batch <= 0 || n_level_nodes <= 0) return hipSuccess;
    if (n > bd_matrix_max_order() || n > a.ld || batch > 0x7fffffff || n_level_nodes > 65535) return hipErrorInvalidValue;
    dim3 grid((unsigned)batch, (unsigned)n_level_nodes), block(64);
#define CAFE_FL_CASE(EV)                                                                     \
    if (n <= 64 * EV) {                                                                      \
        (void)hipGetLastError();                                                             \
        hipLaunchKernelGGL((family_lambda_lm_kernel<EV>), grid, block, 0, stream, a);        \
        return hipGetLastError();                                                            \
    }
    CAFE_FL_CASE(2)
    CAFE_FL_CASE(4)
    CAFE_FL_CASE(6)
    CAFE_FL_CASE(8)
    CAFE_FL_CASE(10)
    CAFE_FL_CASE(12)
    CAFE_FL_CASE(14)
    CAFE_FL_CASE(16)
    CAFE_FL_CASE(20)
    CAFE_FL_CASE(24)
    CAFE_FL_CASE(28)
    CAFE_FL_CASE(32)
#undef CAFE_FL_CASE
    return hipErrorInvalidValue;
}

}  // namespace cafe
