// The row step of the birth-death recurrence, shared by K1 (bd_matrix_build.h: the rows are stored) and the per-family kernel
// (family_lambda_kernel.h: a row is consumed in a dot product and never stored), for equal and for separate birth and death rates.
//
// The single-lineage law of the linear birth-death process over a branch is
//     p1(0) = a,   p1(k) = (1-a)(1-b) b^(k-1)  (k >= 1)
// (a, b: bd_rates in cafe_kernels.h; lambda = mu gives a = b = lambda t / (1 + lambda t), the critical process), and row s of P
// is row s-1 convolved with p1.  One 64-lane wave holds a row of P: lane l owns E consecutive columns.  A step turns row s-1
// into row s,
//     h(c) = P[s-1][c-1] + b h(c-1),        P[s][c] = a P[s-1][c] + (1-a)(1-b) h(c),     clamped to [0,1]:
// the h recurrence and the scan run on the ratio b of the geometric tail, the outer FMA on a.  That is E local FMAs, a scan over
// the 64 lane aggregates with the constant ratio b^E, and E fix-up FMAs.  All terms are non-negative (no cancellation).  The
// scan runs on DPP moves only (no LDS crossbar, no barrier): four Kogge-Stone steps inside each row of 16 lanes
// (row_shr:1,2,4,8), then the row totals are carried over with row_bcast:15 and row_bcast:31 times a per-lane power of the
// ratio; the neighbour values (last column of the lane to the left, the carry) are wave_shr:1.
//
// The step is one function on one constants type.  The equal-rate form of the constants holds a alone and answers it for both
// ratios, so it stores and keeps live no second constant; with a == b every operand of every instruction of the two-rate form,
// and so every bit of the result, is the equal-rate form's.
#pragma once

#include <hip/hip_runtime.h>

namespace cafe {

// DPP move of a double (two 32-bit halves); lanes without a source read 0
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_move(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
    return __hiloint2double(hi, lo);
}
constexpr int kDppRowShr1 = 0x111, kDppRowShr2 = 0x112, kDppRowShr4 = 0x114, kDppRowShr8 = 0x118;
constexpr int kDppWaveShr1 = 0x138, kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143;

// The two ratios of a row step.  Equal rates: one number, no second member.
template <bool TWO_RATES>
struct BdRowRates {
    double a;
    __device__ __forceinline__ void set(double outer_, double) { a = outer_; }
    __device__ __forceinline__ double outer() const { return a; }
    __device__ __forceinline__ double tail() const { return a; }
};
template <>
struct BdRowRates<true> {
    double a, b;                         // p1(0); the ratio of the geometric tail
    __device__ __forceinline__ void set(double outer_, double tail_) { a = outer_; b = tail_; }
    __device__ __forceinline__ double outer() const { return a; }
    __device__ __forceinline__ double tail() const { return b; }
};

// What a wave's row steps share: the ratios, and the powers of the tail ratio a lane needs
template <int E, bool TWO_RATES>
struct BdRowConsts : BdRowRates<TWO_RATES> {
    double q;                            // (1-a)(1-b)
    double tpow[E];                      // tail^(i+1)
    double ratio[4];                     // (tail^E)^(2^d): the in-row scan steps
    double w15, w31;                     // what a lane of rows 1, 3 (rows 2, 3) adds of the total that lane 15 of the row before (lane 31) holds

    // equal rates: `tail` is not read
    __device__ __forceinline__ void init(double outer, double tail, double q_, int lane) {
        this->set(outer, tail);
        q = q_;
        tpow[0] = this->tail();
#pragma unroll
        for (int i = 1; i < E; ++i) tpow[i] = tpow[i - 1] * this->tail();
        ratio[0] = tpow[E - 1];
#pragma unroll
        for (int d = 1; d < 4; ++d) ratio[d] = ratio[d - 1] * ratio[d - 1];
        w15 = pow(tpow[E - 1], (double)((lane & 15) + 1));
        w31 = lane >= 32 ? pow(tpow[E - 1], (double)(lane - 31)) : 0.0;
    }
};

// p[i] = P[row-1][c0 + i] -> P[row][c0 + i].  left0: what lane 0 sees to the left of its first column (P[row-1][c0 - 1]:
// 0 when lane 0 owns column 0; column 0 of the row before of the process the step runs, outer^(row-1), when it owns column 1).
// QM: qm[i] is the lane's per-column (1-a)(1-b), zero for the columns past the matrix (they then stay exactly 0); otherwise every
// column uses k.q and qm is not read.
template <int E, bool QM, bool TWO_RATES>
__device__ __forceinline__ void bd_row_step(const BdRowConsts<E, TWO_RATES>& k, const double* __restrict__ qm, double left0, int lane, double (&p)[E]) {
    double left = dpp_move<kDppWaveShr1>(p[E - 1]);
    if (lane == 0) left = left0;
    double h[E];
    h[0] = left;
#pragma unroll
    for (int i = 1; i < E; ++i) h[i] = fma(k.tail(), h[i - 1], p[i - 1]);
    double S = h[E - 1];             // inclusive scan of the lane totals with ratio tail^E
    S = fma(k.ratio[0], dpp_move<kDppRowShr1>(S), S);          // lanes without a source add ratio * 0
    S = fma(k.ratio[1], dpp_move<kDppRowShr2>(S), S);
    S = fma(k.ratio[2], dpp_move<kDppRowShr4>(S), S);
    S = fma(k.ratio[3], dpp_move<kDppRowShr8>(S), S);
    S = fma(k.w15, dpp_move<kDppRowBcast15, 0xa>(S), S);       // rows 1 and 3 take the total of rows 0 and 2
    S = fma(k.w31, dpp_move<kDppRowBcast31, 0xc>(S), S);       // rows 2 and 3 take the total of rows 0..1
    const double carry = dpp_move<kDppWaveShr1>(S);            // lane 0: 0
#pragma unroll
    for (int i = 0; i < E; ++i) {
        double hh = fma(k.tpow[i], carry, h[i]);
        double v = fma(k.outer(), p[i], (QM ? qm[i] : k.q) * hh);
        v = v < 1.0 ? v : 1.0;
        p[i] = v > 0.0 ? v : 0.0;
    }
}

}  // namespace cafe
