// The body of K1 bd_matrix_build: one function template on the slot type for both rate models (bd_matrix.hip has the derivation
// and the mapping; it instantiates SlotParam, bd_matrix_lm.hip SlotParamLM).  Kernels, launchers and the one 1/r table.
#pragma once

#include "bd_row.h"
#include "cafe_kernels.h"

// diagnostic: -D'CAFE_EXPERIMENT_K1_STORE_IF=&& n < 0' builds K1 without its global stores (the matrices are wrong): what is
// left is the latency chain of the row steps, DESIGN.md section 3 K1
#ifndef CAFE_EXPERIMENT_K1_STORE_IF
#define CAFE_EXPERIMENT_K1_STORE_IF
#endif

namespace cafe {

namespace {
// 1 / r for the k-major scaling P[s][c] = (s/c) P[c][s]: the division (v_rcp_f64 + two scales + four FMAs + fix-up) sat in
// every row step; the correctly rounded quotient is the same number whoever divides, so it is folded at compile time and read
// with a scalar load (r is uniform).  Orders go up to bd_matrix_max_order() = 2048.
struct InvTable {
    double v[2048];
    constexpr InvTable() : v() {
        for (int i = 1; i < 2048; ++i) v[i] = 1.0 / (double)i;
    }
};
__constant__ InvTable kInvR = InvTable();
}  // namespace

// One matrix on one wave.  Slot decides the rate model: SlotParam (lambda = mu: tail ratio = alpha, q = (1-alpha)^2, no second
// constant) or SlotParamLM (alpha, beta, q = (1-alpha)(1-beta)); slot_tail / slot_q (cafe_kernels.h) are all that differs.
template <class Slot, int E, bool KMAJOR>
__device__ __forceinline__ void bd_matrix_build_one(const MatrixPool& pool, const Slot sp, int slot) {
    const int lane = threadIdx.x;
    double* __restrict__ P = pool.base + (int64_t)slot * pool.stride;
    const int ld = pool.ld;
    const int n = pool.n;                             // matrix order N (sizes 0..N-1)
    const int n_rows = KMAJOR ? pool.rows : n;        // rows to write
    const int k_valid = KMAJOR ? pool.k_valid : n;    // recurrence rows that are ever read
    constexpr int e_base = KMAJOR ? 1 : 0;            // first owned column of lane 0
    const int c0 = e_base + lane * E;                 // owned columns c0 .. c0+E-1 of the current P row
    const int j0 = lane * E;                          // where they are stored
    const double a = sp.alpha, q = slot_q(sp);
    // the recurrence this layout runs: row-major the process itself, k-major the EXCHANGED one (tail ratio alpha, extinction
    // beta; the header of bd_matrix.hip).  Equal rates: the same process.
    const double outer = KMAJOR ? slot_tail(sp) : sp.alpha, tail = KMAJOR ? sp.alpha : slot_tail(sp);

    BdRowConsts<E, Slot::two_rates> rc;  // the powers of the tail ratio the row step needs (bd_row.h)
    rc.init(outer, tail, q, lane);

    // Columns past the matrix (c0 + i >= n: the tail of the last lanes) must be stored as zeros.  Up to E = 16 they ARE zeros: the
    // lane multiplies h by a per-element q that is 0 there, so p stays exactly 0 (a p + 0 h) and nothing is masked per
    // row step -- 2 E selects less of its ~200 instructions; columns inside the matrix see the same operands as before.  Wider
    // E keeps the selects (E more live doubles would spill).
    constexpr bool QM = E <= 16;
    double qm[QM ? E : 1];
#pragma unroll
    for (int i = 0; i < (QM ? E : 1); ++i) qm[i] = (c0 + i < n) ? q : 0.0;
    double p[E];                         // row of the recurrence, columns c0 + i
    // k-major only: lane 0's left neighbour is column 0 of the process the recurrence runs -- the exchanged one, outer^row --
    // which "exchange the two" does not give
    double p0 = 1.0;
#pragma unroll
    for (int i = 0; i < E; ++i) p[i] = (c0 + i == 0) ? 1.0 : 0.0;

    // A lane owns E consecutive columns (what the scan needs); stored from there, an instruction would write 64 pieces of
    // 16 bytes 8*E bytes apart.  The row is turned through LDS instead (one wave per block: a wait on the LDS counter is
    // the only synchronisation) and leaves as 1 KB contiguous per store instruction.
    __shared__ double2 rowbuf[64 * E / 2];
    auto store_row = [&](int r, const double* v) {
        if constexpr (E <= 4) {
            // small orders: a matrix is a chain of short row steps, not a stream of lines, and the LDS round trip with its two
            // waits is a seventh of a step (mammals K1 59.5 -> 51 us).  The lane stores its own columns (pieces 8*E bytes apart: the row is 1-2 KB).
            double2* row = reinterpret_cast<double2*>(P + (int64_t)r * ld);
#pragma unroll
            for (int i = 0; i < E; i += 2) {
                double2 w;
                w.x = (QM || c0 + i < n) ? v[i] : 0.0;
                w.y = (QM || c0 + i + 1 < n) ? v[i + 1] : 0.0;
                if (j0 + i < ld CAFE_EXPERIMENT_K1_STORE_IF) row[(j0 + i) >> 1] = w;
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
            if (2 * q < ld CAFE_EXPERIMENT_K1_STORE_IF) row[q] = rowbuf[q];      // (non-temporal stores measured: 1.24 -> 1.29-1.33 ms at order 751)
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
        if (!pool.ext) return;                         // (uniform) orders below 256 publish no extents: nothing to track in the row step
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

    if (sp.zero) {                       // saturated / degenerate (slot_param, slot_param_lm): every entry with parent size >= 1 is 0
        if (!KMAJOR) { store_row(0, p); note(0, p); }    // row-major keeps P's row 0 = e_0; k-major never holds it
        for (int r = KMAJOR ? 0 : 1; r < n_rows; ++r) store_row(r, z);
        publish_extents();               // all blocks empty
        return;
    }

    if (KMAJOR) {
        // Pt[0][j] = P[j+1][0] = a^(j+1): the extinction probability of the process ITSELF, from its own alpha and not the
        // exchanged process's
        double v[E];
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
        bd_row_step<E, QM>(rc, qm, KMAJOR ? p0 : 0.0, lane, p);
        p0 *= outer;
        if (KMAJOR) {
            const double inv_r = kInvR.v[r];               // = 1.0 / (double)r, bit for bit
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

template <class Slot, int E, bool KMAJOR>
__global__ __launch_bounds__(64) void bd_matrix_build_kernel(MatrixPool pool, const Slot* __restrict__ slots, int n_slots) {
    const int slot = blockIdx.x;
    if (slot >= n_slots) return;
    bd_matrix_build_one<Slot, E, KMAJOR>(pool, slots[slot], slot);
}

// both pools of a scorer call in one launch: each matrix is a latency-bound chain of N row steps on one wave, so the
// row-major and the k-major matrices should be in flight together rather than one launch after the other
template <class Slot, int E>
__global__ __launch_bounds__(64) void bd_matrix_build_both_kernel(MatrixPool pool, MatrixPool kpool, const Slot* __restrict__ slots,
                                                                  const Slot* __restrict__ kslots, int n_slots, int n_kslots) {
    const int b = blockIdx.x;                          // uniform per wave: no divergence
    if (b < n_kslots) bd_matrix_build_one<Slot, E, true>(kpool, kslots[b], b);          // the longer chains first
    else if (b - n_kslots < n_slots) bd_matrix_build_one<Slot, E, false>(pool, slots[b - n_kslots], b - n_kslots);
}

template <class Slot, bool KMAJOR>
hipError_t launch_layout(const MatrixPool& pool, const Slot* d_slots, int n_slots, hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    const int cols = KMAJOR ? pool.n - 1 : pool.n;      // owned columns needed: c = e_base .. n-1
    if (cols > bd_matrix_max_order() || (pool.ld & 1)) return hipErrorInvalidValue;
    dim3 grid(n_slots), block(64);
    return for_lane_width(cols, [&](auto e) {
        (void)hipGetLastError();
        hipLaunchKernelGGL((bd_matrix_build_kernel<Slot, decltype(e)::value, KMAJOR>), grid, block, 0, stream, pool, d_slots, n_slots);
        return hipGetLastError();
    });
}

template <class Slot>
hipError_t launch_bd_matrix_build(const MatrixPool& pool, const Slot* d_slots, int n_slots, hipStream_t stream) {
    return pool.kmajor ? launch_layout<Slot, true>(pool, d_slots, n_slots, stream) : launch_layout<Slot, false>(pool, d_slots, n_slots, stream);
}

template <class Slot>
hipError_t launch_bd_matrix_build_both(const MatrixPool& pool, const MatrixPool& kpool, const Slot* d_slots, const Slot* d_kslots, int n_slots,
                                       int n_kslots, hipStream_t stream) {
    if (n_slots <= 0 || n_kslots <= 0) {               // one layout only: the single-pool launch
        hipError_t e = launch_bd_matrix_build(pool, d_slots, n_slots, stream);
        return e != hipSuccess ? e : launch_bd_matrix_build(kpool, d_kslots, n_kslots, stream);
    }
    const int cols = pool.n;
    if (cols > bd_matrix_max_order() || (pool.ld & 1) || (kpool.ld & 1) || pool.n != kpool.n) return hipErrorInvalidValue;
    dim3 grid(n_slots + n_kslots), block(64);
    return for_lane_width(cols, [&](auto e) {
        (void)hipGetLastError();
        hipLaunchKernelGGL((bd_matrix_build_both_kernel<Slot, decltype(e)::value>), grid, block, 0, stream, pool, kpool, d_slots, d_kslots, n_slots,
                           n_kslots);
        return hipGetLastError();
    });
}

}  // namespace cafe
