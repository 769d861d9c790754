// The row step of the birth-death recurrence with SEPARATE birth and death rates (bd_matrix_lm.hip has the derivation): the
// two-rate twin of bd_row_step (bd_row.h), which stays what K1 and the per-family kernel share for lambda = mu.
//
// The single-lineage law is p1(0) = a, p1(k) = (1-a)(1-b) b^(k-1), so a step turns row s-1 into row s with
//     h(c) = P[s-1][c-1] + b h(c-1),        P[s][c] = a P[s-1][c] + (1-a)(1-b) h(c),     clamped to [0,1]:
// the scan ratio and the h recurrence run on b, the outer FMA on a.  Same mapping (lane l owns E consecutive columns), same
// DPP-only scan, same instruction count as bd_row_step: one more constant is live.  With a == b every operand, and so every
// bit of the result, is bd_row_step's.
#pragma once

#include "bd_row.h"

namespace cafe {

// What a wave's row steps share: a, and the powers of b a lane needs
template <int E>
struct BdRowConstsLM {
    double a, b, q;                      // p1(0); the ratio of the geometric tail; (1-a)(1-b)
    double bpow[E];                      // b^(i+1)
    double ratio[4];                     // (b^E)^(2^d): the in-row scan steps
    double w15, w31;                     // as BdRowConsts, on b

    __device__ __forceinline__ void init(double outer, double tail, double q_, int lane) {
        a = outer; b = tail; q = q_;
        bpow[0] = b;
#pragma unroll
        for (int i = 1; i < E; ++i) bpow[i] = bpow[i - 1] * b;
        ratio[0] = bpow[E - 1];
#pragma unroll
        for (int d = 1; d < 4; ++d) ratio[d] = ratio[d - 1] * ratio[d - 1];
        w15 = pow(bpow[E - 1], (double)((lane & 15) + 1));
        w31 = lane >= 32 ? pow(bpow[E - 1], (double)(lane - 31)) : 0.0;
    }
};

// p[i] = P[row-1][c0 + i] -> P[row][c0 + i].  left0: what lane 0 sees to the left of its first column (0 when lane 0 owns
// column 0; the process's column 0 of the row before when it owns column 1).  QM: qm[i] is the lane's per-column (1-a)(1-b),
// zero for the columns past the matrix (they then stay exactly 0); otherwise every column uses k.q and qm is not read.
template <int E, bool QM>
__device__ __forceinline__ void bd_row_step_lm(const BdRowConstsLM<E>& k, const double* __restrict__ qm, double left0, int lane, double (&p)[E]) {
    double left = dpp_move<kDppWaveShr1>(p[E - 1]);
    if (lane == 0) left = left0;
    double h[E];
    h[0] = left;
#pragma unroll
    for (int i = 1; i < E; ++i) h[i] = fma(k.b, h[i - 1], p[i - 1]);
    double S = h[E - 1];             // inclusive scan of the lane totals with ratio b^E
    S = fma(k.ratio[0], dpp_move<kDppRowShr1>(S), S);          // lanes without a source add ratio * 0
    S = fma(k.ratio[1], dpp_move<kDppRowShr2>(S), S);
    S = fma(k.ratio[2], dpp_move<kDppRowShr4>(S), S);
    S = fma(k.ratio[3], dpp_move<kDppRowShr8>(S), S);
    S = fma(k.w15, dpp_move<kDppRowBcast15, 0xa>(S), S);       // rows 1 and 3 take the total of rows 0 and 2
    S = fma(k.w31, dpp_move<kDppRowBcast31, 0xc>(S), S);       // rows 2 and 3 take the total of rows 0..1
    const double carry = dpp_move<kDppWaveShr1>(S);            // lane 0: 0
#pragma unroll
    for (int i = 0; i < E; ++i) {
        double hh = fma(k.bpow[i], carry, h[i]);
        double v = fma(k.a, p[i], (QM ? qm[i] : k.q) * hh);
        v = v < 1.0 ? v : 1.0;
        p[i] = v > 0.0 ? v : 0.0;
    }
}

}  // namespace cafe
