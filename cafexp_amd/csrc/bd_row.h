// The row step of the birth-death recurrence (bd_matrix.hip has the derivation), shared by K1 (bd_matrix.hip: the rows are
// stored) and the per-family kernel (family_lambda.hip: a row is consumed in a dot product and never stored).
//
// One 64-lane wave holds a row of P: lane l owns E consecutive columns.  A step turns row s-1 into row s,
//     h(c) = P[s-1][c-1] + a h(c-1),        P[s][c] = a P[s-1][c] + (1-a)^2 h(c),     clamped to [0,1],
// with E local FMAs, a scan over the 64 lane aggregates with the constant ratio a^E, and E fix-up FMAs.  The scan runs on
// DPP moves only (no LDS crossbar, no barrier): four Kogge-Stone steps inside each row of 16 lanes (row_shr:1,2,4,8), then
// the row totals are carried over with row_bcast:15 and row_bcast:31 times a per-lane power of the ratio; the neighbour
// values (last column of the lane to the left, the carry) are wave_shr:1.
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

// What a wave's row steps share: the powers of a = lambda t / (1 + lambda t) a lane needs
template <int E>
struct BdRowConsts {
    double a, q;                         // a, (1-a)^2
    double apow[E];                      // a^(i+1)
    double ratio[4];                     // (a^E)^(2^d): the in-row scan steps
    double w15, w31;                     // what a lane of rows 1, 3 (rows 2, 3) adds of the total that lane 15 of the row before (lane 31) holds

    __device__ __forceinline__ void init(double alpha, double oma2, int lane) {
        a = alpha; q = oma2;
        apow[0] = a;
#pragma unroll
        for (int i = 1; i < E; ++i) apow[i] = apow[i - 1] * a;
        ratio[0] = apow[E - 1];
#pragma unroll
        for (int d = 1; d < 4; ++d) ratio[d] = ratio[d - 1] * ratio[d - 1];
        w15 = pow(apow[E - 1], (double)((lane & 15) + 1));
        w31 = lane >= 32 ? pow(apow[E - 1], (double)(lane - 31)) : 0.0;
    }
};

// p[i] = P[row-1][c0 + i] -> P[row][c0 + i].  left0: what lane 0 sees to the left of its first column (P[row-1][c0 - 1]:
// 0 when lane 0 owns column 0, a^(row-1) when it owns column 1).  QM: qm[i] is the lane's per-column (1-a)^2, zero for the
// columns past the matrix (they then stay exactly 0); otherwise every column uses k.q and qm is not read.
template <int E, bool QM>
__device__ __forceinline__ void bd_row_step(const BdRowConsts<E>& k, const double* __restrict__ qm, double left0, int lane, double (&p)[E]) {
    double left = dpp_move<kDppWaveShr1>(p[E - 1]);
    if (lane == 0) left = left0;
    double h[E];
    h[0] = left;
#pragma unroll
    for (int i = 1; i < E; ++i) h[i] = fma(k.a, h[i - 1], p[i - 1]);
    double S = h[E - 1];             // inclusive scan of the lane totals with ratio a^E
    S = fma(k.ratio[0], dpp_move<kDppRowShr1>(S), S);          // lanes without a source add ratio * 0
    S = fma(k.ratio[1], dpp_move<kDppRowShr2>(S), S);
    S = fma(k.ratio[2], dpp_move<kDppRowShr4>(S), S);
    S = fma(k.ratio[3], dpp_move<kDppRowShr8>(S), S);
    S = fma(k.w15, dpp_move<kDppRowBcast15, 0xa>(S), S);       // rows 1 and 3 take the total of rows 0 and 2
    S = fma(k.w31, dpp_move<kDppRowBcast31, 0xc>(S), S);       // rows 2 and 3 take the total of rows 0..1
    const double carry = dpp_move<kDppWaveShr1>(S);            // lane 0: 0
#pragma unroll
    for (int i = 0; i < E; ++i) {
        double hh = fma(k.apow[i], carry, h[i]);
        double v = fma(k.a, p[i], (QM ? qm[i] : k.q) * hh);
        v = v < 1.0 ? v : 1.0;
        p[i] = v > 0.0 ? v : 0.0;
    }
}

}  // namespace cafe
