// K1 with separate birth and death rates: all transition matrices of one call under the linear birth-death process with
// birth rate lambda and death rate mu per lineage.  bd_matrix.hip is the lambda = mu kernel and stays what every call without
// death rates runs (cafe_set_death_rates); this file is its two-rate twin, with a row step of its own (bd_row_lm.h).
//
// The single-lineage law over a branch of length t is
//     p1(0) = a,   p1(k) = (1-a)(1-b) b^(k-1)  (k >= 1),
//     a = mu (E-1) / (lambda E - mu),   b = lambda (E-1) / (lambda E - mu),   E = exp((lambda - mu) t)
// (cafe_bd_rates evaluates a and b on the host; both tend to lambda t / (1 + lambda t) as mu -> lambda), and row s of P is
// row s-1 convolved with p1, a first-order linear recurrence along the row:
//     h(c) = P[s-1][c-1] + b h(c-1),        P[s][c] = a P[s-1][c] + (1-a)(1-b) h(c).
// All terms are non-negative, O(N^2) per matrix.  Kept from K1: one 64-lane wave per matrix, E columns per lane, the DPP-only
// scan, both layouts and the two-pool launch, the LDS turn of a row for E > 4, exact zeros in the columns past the matrix,
// the [0,1] clamp, row 0 = e_0, rows s >= 1 zero for a slot marked `zero`, and the non-zero extents of both kinds.
//
// The k-major layout is again written without a transpose.  The process is reversible with respect to
// pi(n) = (lambda/mu)^n / n, and exchanging the rates exchanges a and b, so
//     P_{lambda,mu}[s][c] = (s/c) P_{mu,lambda}[c][s]        (s, c >= 1):
// Pt's row c is row c of the EXCHANGED process (tail ratio a, extinction b) scaled by s/c -- the power of lambda/mu is folded
// into the recurrence and never formed.  What does not follow from "exchange the two":
//   - Pt's row 0 is P[s][0] = a^s, the extinction probability of the process itself;
//   - lane 0's left neighbour is column 0 of the exchanged process, b^(r-1);
// everything else is the row-major code with the other constant.
#include "bd_row_lm.h"
#include "cafe_kernels.h"

namespace cafe {

namespace {
// 1 / r for the k-major scaling, folded at compile time (bd_matrix.hip: the correctly rounded quotient, read with a scalar load)
struct InvTableLM {
    double v[2048];
    constexpr InvTableLM() : v() {
        for (int i = 1; i < 2048; ++i) v[i] = 1.0 / (double)i;
    }
};
__constant__ InvTableLM kInvRLM = InvTableLM();
}  // namespace

template <int E, bool KMAJOR>
__device__ __forceinline__ void bd_lm_build_one(const MatrixPool& pool, const SlotParamLM sp, int slot) {
    const int lane = threadIdx.x;
    double* __restrict__ P = pool.base + (int64_t)slot * pool.stride;
    const int ld = pool.ld;
    const int n = pool.n;                             // matrix order N (sizes 0..N-1)
    const int n_rows = KMAJOR ? pool.rows : n;        // rows to write
    const int k_valid = KMAJOR ? pool.k_valid : n;    // recurrence rows that are ever read
    constexpr int e_base = KMAJOR ? 1 : 0;            // first owned column of lane 0
    const int c0 = e_base + lane * E;                 // owned columns c0 .. c0+E-1 of the current P row
    const int j0 = lane * E;                          // where they are stored
    const double a = sp.alpha, q = sp.q;
    // the recurrence this layout runs: row-major the process itself, k-major the exchanged one
    const double outer = KMAJOR ? sp.beta : sp.alpha, tail = KMAJOR ? sp.alpha : sp.beta;

    BdRowConstsLM<E> rc;                 // the powers of the tail ratio the row step needs (bd_row_lm.h)
    rc.init(outer, tail, q, lane);

    // columns past the matrix are stored as zeros: up to E = 16 through a per-element q that is 0 there, wider E with selects
    // (bd_matrix.hip)
    constexpr bool QM = E <= 16;
    double qm[QM ? E : 1];
#pragma unroll
    for (int i = 0; i < (QM ? E : 1); ++i) qm[i] = (c0 + i < n) ? q : 0.0;
    double p[E];                         // row of the recurrence, columns c0 + i
    double p0 = 1.0;                     // column 0 of the exchanged process, outer^row (k-major only: lane 0's left neighbour)
#pragma unroll
    for (int i = 0; i < E; ++i) p[i] = (c0 + i == 0) ? 1.0 : 0.0;

    // the row is turned through LDS (one wave per block: a wait on the LDS counter is the only synchronisation) and leaves as
    // 1 KB contiguous per store instruction; E <= 4: the lane stores its own columns (bd_matrix.hip)
    __shared__ double2 rowbuf[64 * E / 2];
    auto store_row = [&](int r, const double* v) {
        if constexpr (E <= 4) {
            double2* row = reinterpret_cast<double2*>(P + (int64_t)r * ld);
#pragma unroll
            for (int i = 0; i < E; i += 2) {
                double2 w;
                w.x = (QM || c0 + i < n) ? v[i] : 0.0;
                w.y = (QM || c0 + i + 1 < n) ? v[i + 1] : 0.0;
                if (j0 + i < ld) row[(j0 + i) >> 1] = w;
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < E; i += 2) {
            double2 w;
            w.x = (QM || c0 + i < n) ? v[i] : 0.0;
            w.y = (QM || c0 + i + 1 < n) ? v[i + 1] : 0.0;
            rowbuf[(j0 + i) >> 1] = w;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): every lane's part of the row is in LDS
        __asm__ volatile("" ::: "memory");
        double2* row = reinterpret_cast<double2*>(P + (int64_t)r * ld);
#pragma unroll
        for (int i = 0; i < E / 2; ++i) {
            const int q = lane + 64 * i;                 // 16-byte piece of the row
            if (2 * q < ld) row[q] = rowbuf[q];
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);          // the pieces are in registers before the next row overwrites the buffer
        __asm__ volatile("" ::: "memory");
    };

    double z[E];
#pragma unroll
    for (int i = 0; i < E; ++i) z[i] = 0.0;

    // k-major: the non-zero extent (first / last contraction index) of every block of 16 stored columns, for K2
    __shared__ int ext_lo[128], ext_hi[128];
    int first_nz = 0x7fffffff, last_nz = -1;          // over this lane's columns
    int col_first[KMAJOR ? 1 : E], col_last[KMAJOR ? 1 : E];   // row-major: first / last row (parent size) with a non-zero entry, per owned column
#pragma unroll
    for (int i = 0; i < (KMAJOR ? 1 : E); ++i) { col_first[i] = 0x7fffffff; col_last[i] = -1; }
    auto note = [&](int r, const double* v) {
        if (!pool.ext) return;                         // (uniform) orders below 256 publish no extents
        if (KMAJOR) {
            bool any = false;
#pragma unroll
            for (int i = 0; i < E; ++i) any = any || ((QM || c0 + i < n) && v[i] != 0.0);
            if (any) { first_nz = first_nz < r ? first_nz : r; last_nz = r; }
        } else {
#pragma unroll
            for (int i = 0; i < (KMAJOR ? 1 : E); ++i)
                if (v[i] != 0.0) { col_first[i] = col_first[i] < r ? col_first[i] : r; col_last[i] = r; }
        }
    };
    auto publish_extents = [&]() {
        if (!pool.ext) return;
        if (!KMAJOR) {                                 // per column x of P: rows s with P[s][x] != 0 (the support of a leaf's factor)
            int32_t* out = pool.ext + (int64_t)slot * pool.ext_blocks * 2;
#pragma unroll
            for (int i = 0; i < (KMAJOR ? 1 : E); ++i)
                if (c0 + i < n) { out[2 * (c0 + i)] = col_first[i]; out[2 * (c0 + i) + 1] = col_last[i]; }
            return;
        }
        const int nb = pool.ext_blocks;
        for (int b = lane; b < nb; b += 64) { ext_lo[b] = 0x7fffffff; ext_hi[b] = -1; }
        __syncthreads();                               // one wave per block: orders the LDS initialisation
        if (last_nz >= 0 && j0 < n - 1) {
            const int b_lo = j0 >> 4, b_hi = min(j0 + E - 1, n - 2) >> 4;
            for (int b = b_lo; b <= b_hi && b < nb; ++b) { atomicMin(&ext_lo[b], first_nz); atomicMax(&ext_hi[b], last_nz); }
        }
        __syncthreads();
        int32_t* out = pool.ext + (int64_t)slot * nb * 2;
        for (int b = lane; b < nb; b += 64) { out[2 * b] = ext_lo[b]; out[2 * b + 1] = ext_hi[b]; }
    };

    if (sp.zero) {                       // saturated / degenerate (cafe_bd_rates): every entry with parent size >= 1 is 0
        if (!KMAJOR) { store_row(0, p); note(0, p); }    // row-major keeps P's row 0 = e_0; k-major never holds it
        for (int r = KMAJOR ? 0 : 1; r < n_rows; ++r) store_row(r, z);
        publish_extents();               // all blocks empty
        return;
    }

    if (KMAJOR) {
        double v[E];                     // Pt[0][j] = P[j+1][0] = a^(j+1): the process's own extinction probability, not the exchanged one's
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (!QM || c0 + i < n) ? pow(a, (double)(c0 + i)) : 0.0;
        store_row(0, v);
        note(0, v);
    } else {
        store_row(0, p);
        note(0, p);
    }

    for (int r = 1; r < n_rows; ++r) {
        if (r >= k_valid || r >= n) {    // contraction rows past M (or past the matrix) are never read: keep them 0
            store_row(r, z);
            continue;
        }
        bd_row_step_lm<E, QM>(rc, qm, KMAJOR ? p0 : 0.0, lane, p);
        p0 *= outer;
        if (KMAJOR) {
            const double inv_r = kInvRLM.v[r];             // = 1.0 / (double)r, bit for bit
            double v[E];
#pragma unroll
            for (int i = 0; i < E; ++i) {
                double t = p[i] * ((double)(c0 + i) * inv_r);     // P_{lambda,mu}[s][c] = (s/c) P_{mu,lambda}[c][s]
                v[i] = t < 1.0 ? t : 1.0;
            }
            store_row(r, v);
            note(r, v);
        } else {
            store_row(r, p);
            note(r, p);
        }
    }
    publish_extents();
}

template <int E, bool KMAJOR>
__global__ __launch_bounds__(64) void bd_lm_kernel(MatrixPool pool, const SlotParamLM* __restrict__ slots, int n_slots) {
    const int slot = blockIdx.x;
    if (slot >= n_slots) return;
    bd_lm_build_one<E, KMAJOR>(pool, slots[slot], slot);
}

// both pools of a scorer call in one launch (bd_matrix.hip): the longer k-major chains first
template <int E>
__global__ __launch_bounds__(64) void bd_lm_both_kernel(MatrixPool pool, MatrixPool kpool, const SlotParamLM* __restrict__ slots,
                                                        const SlotParamLM* __restrict__ kslots, int n_slots, int n_kslots) {
    const int b = blockIdx.x;                          // uniform per wave: no divergence
    if (b < n_kslots) bd_lm_build_one<E, true>(kpool, kslots[b], b);
    else if (b - n_kslots < n_slots) bd_lm_build_one<E, false>(pool, slots[b - n_kslots], b - n_kslots);
}

template <bool KMAJOR>
static hipError_t launch_layout_lm(const MatrixPool& pool, const SlotParamLM* d_slots, int n_slots, hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    const int cols = KMAJOR ? pool.n - 1 : pool.n;      // owned columns needed: c = e_base .. n-1
    if (cols > bd_matrix_max_order() || (pool.ld & 1)) return hipErrorInvalidValue;
    dim3 grid(n_slots), block(64);
#define CAFE_BD_CASE(EV)                                                                                \
    if (cols <= 64 * EV) {                                                                              \
        (void)hipGetLastError();                                                                        \
        hipLaunchKernelGGL((bd_lm_kernel<EV, KMAJOR>), grid, block, 0, stream, pool, d_slots, n_slots); \
        return hipGetLastError();                                                                       \
    }
    CAFE_BD_CASE(2)
    CAFE_BD_CASE(4)
    CAFE_BD_CASE(6)
    CAFE_BD_CASE(8)
    CAFE_BD_CASE(10)
    CAFE_BD_CASE(12)
    CAFE_BD_CASE(14)
    CAFE_BD_CASE(16)
    CAFE_BD_CASE(20)
    CAFE_BD_CASE(24)
    CAFE_BD_CASE(28)
    CAFE_BD_CASE(32)
#undef CAFE_BD_CASE
    return hipErrorInvalidValue;
}

hipError_t launch_bd_lm_build(const MatrixPool& pool, const SlotParamLM* d_slots, int n_slots, hipStream_t stream) {
    return pool.kmajor ? launch_layout_lm<true>(pool, d_slots, n_slots, stream) : launch_layout_lm<false>(pool, d_slots, n_slots, stream);
}

hipError_t launch_bd_lm_build_both(const MatrixPool& pool, const MatrixPool& kpool, const SlotParamLM* d_slots, const SlotParamLM* d_kslots,
                                   int n_slots, int n_kslots, hipStream_t stream) {
    if (n_slots <= 0 || n_kslots <= 0) {               // one layout only: the single-pool launch
        hipError_t e = launch_bd_lm_build(pool, d_slots, n_slots, stream);
        return e != hipSuccess ? e : launch_bd_lm_build(kpool, d_kslots, n_kslots, stream);
    }
    const int cols = pool.n;
    if (cols > bd_matrix_max_order() || (pool.ld & 1) || (kpool.ld & 1) || pool.n != kpool.n) return hipErrorInvalidValue;
    dim3 grid(n_slots + n_kslots), block(64);
#define CAFE_BD_CASE(EV)                                                                                                          \
    if (cols <= 64 * EV) {                                                                                                        \
        (void)hipGetLastError();                                                                                                  \
        hipLaunchKernelGGL((bd_lm_both_kernel<EV>), grid, block, 0, stream, pool, kpool, d_slots, d_kslots, n_slots, n_kslots);   \
        return hipGetLastError();                                                                                                 \
    }
    CAFE_BD_CASE(2)
    CAFE_BD_CASE(4)
    CAFE_BD_CASE(6)
    CAFE_BD_CASE(8)
    CAFE_BD_CASE(10)
    CAFE_BD_CASE(12)
    CAFE_BD_CASE(14)
    CAFE_BD_CASE(16)
    CAFE_BD_CASE(20)
    CAFE_BD_CASE(24)
    CAFE_BD_CASE(28)
    CAFE_BD_CASE(32)
#undef CAFE_BD_CASE
    return hipErrorInvalidValue;
}

}  // namespace cafe
