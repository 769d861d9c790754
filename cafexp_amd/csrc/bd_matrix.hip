// K1 bd_matrix_build: all birth-death transition matrices of one scorer call.
//
// Replaces matrix_cache::precalculate_matrices (src/matrix_cache.cpp:121-171) and, entry by
// entry, the_probability_of_going_from_parent_fam_size_to_c (src/probability.cpp:147) /
// birthdeath_rate_with_log_alpha (src/probability.cpp:101).  The reference evaluates every
// entry as a log-space sum of min(s,c)+1 terms (O(N^3) per matrix).  The closed form it sums is
// the s-fold convolution of the single-lineage law of the critical linear birth-death process,
//     p1(0) = a,   p1(k) = (1-a)^2 a^(k-1)  (k >= 1),    a = lambda t / (1 + lambda t),
// so row s = row s-1 (*) p1, which is a first-order linear recurrence along the row:
//     h(c) = P[s-1][c-1] + a h(c-1),        P[s][c] = a P[s-1][c] + (1-a)^2 h(c).
// All terms are non-negative (no cancellation), O(N^2) per matrix.  The reference's special
// cases are kept: row 0 = e_0 (matrix_cache.cpp:70-77), saturated or degenerate coeff => rows
// s >= 1 are zero (matrix_cache.cpp:153, probability.cpp:154), values clamped to [0,1]
// (probability.cpp:145).
//
// Mapping: ONE 64-lane wave per matrix.  Lane l owns E consecutive columns of the current row
// in registers; a row step is E local FMAs, a scan over the 64 lane aggregates with the constant
// ratio a^E, and E fix-up FMAs.  The scan runs on DPP moves only (no LDS crossbar, no barrier):
// four Kogge-Stone steps inside each row of 16 lanes (row_shr:1,2,4,8), then the row totals are
// carried over with row_bcast:15 and row_bcast:31 times a per-lane power of the ratio; the
// neighbour values (last column of the lane to the left, the carry) are wave_shr:1.  A row step is
// a dependent chain, so its latency is the kernel's time until the HBM write of the pool takes
// over (__shfl_up, which compiles to ds_bpermute, made a step of N = 751 take 2.5 us).  The row steps are sequential; the grid has one wave per (branch, category)
// matrix, so a call with hundreds of matrices fills the chip.  Measured at N = 751, 1320 matrices (tools/k1_time.py): 1.13 ms, of
// which 0.69 ms is the chain of row steps (the build without its stores) and 0.44 ms the LDS turn + the write of 5.8 GB.
//
// Two output layouts:
//   row-major  P[s][c]              -- leaf branches: K3 reads column x of P (P . e_x)
//   k-major    Pt[c][j] = P[j+1][c] -- interior branches: the A operand of K2, contraction index c
//                                      outermost so that an A tile row is contiguous in LDS-DMA order.
// The k-major layout is written without a transpose: the process is reversible with respect to
// pi(n) = 1/n, so P[s][c] = (s/c) P[c][s] for s,c >= 1; Pt's row c is P's row c scaled by s/c
// (one extra rounding), Pt's row 0 is P[s][0] = a^s, and P's row 0 (e_0) is never stored: K2
// copies that row (prune_gemm.hip).
//
// Separate birth and death rates (bd_matrix_lm.hip instantiates the same body on SlotParamLM).  The single-lineage law is then
//     p1(0) = a,   p1(k) = (1-a)(1-b) b^(k-1)  (k >= 1),
//     a = mu (E-1) / (lambda E - mu),   b = lambda (E-1) / (lambda E - mu),   E = exp((lambda - mu) t)
// (bd_rates evaluates a and b on the host; both tend to lambda t / (1 + lambda t) as mu -> lambda), and the recurrence is
//     h(c) = P[s-1][c-1] + b h(c-1),        P[s][c] = a P[s-1][c] + (1-a)(1-b) h(c).
// The process is reversible with respect to pi(n) = (lambda/mu)^n / n, and exchanging the rates exchanges a and b, so
//     P_{lambda,mu}[s][c] = (s/c) P_{mu,lambda}[c][s]        (s, c >= 1):
// Pt's row c is row c of the EXCHANGED process (tail ratio a, extinction b) scaled by s/c -- the power of lambda/mu is folded
// into the recurrence and never formed.  What does not follow from "exchange the two":
//   - Pt's row 0 is P[s][0] = a^s, the extinction probability of the process itself;
//   - lane 0's left neighbour is column 0 of the exchanged process, b^(r-1), and so p0 advances by b;
// everything else is the row-major code with the other constant.
//
// This file: the body (bd_matrix_build.h) instantiated for lambda = mu, what every call without death rates runs.
#include "bd_matrix_build.h"

namespace cafe {

int bd_matrix_max_order() { return 64 * 32; }

template hipError_t launch_bd_matrix_build_both<SlotParam>(const MatrixPool&, const MatrixPool&, const SlotParam*, const SlotParam*, int, int, hipStream_t);
template hipError_t launch_bd_matrix_build<SlotParam>(const MatrixPool&, const SlotParam*, int, hipStream_t);

}  // namespace cafe
