// Internal: what family_lambda.hip (the host frame of both per-family entries) needs of family_lambda_lm.hip (the two-rate twin
// of its branch kernel).  The argument block is FamLamArgs with the two-rate slot: a struct of its own, so that the lambda = mu
// kernel and its arguments stay what they are.
#pragma once

#include "cafe_kernels.h"

namespace cafe {

// The parked dot product of both branch kernels (family_lambda.hip has the reasoning)
constexpr int kPartRows = 16;        // rows whose lane partials are parked before they are summed
constexpr int kPartLd = 65;          // doubles per parked row: 64 lanes + 1, so that the transposed read spreads over the banks

// MIRROR of FamLamArgs (family_lambda.hip) but for the slot type: a change to one belongs in the other
struct FamLamArgsLM {
    const int32_t* nodes;            // the nodes of this level: one unit of work per branch above them
    const int32_t* child_off;        // [n_nodes + 1] children of a node: child_idx[child_off[u] .. child_off[u + 1])
    const int32_t* child_idx;
    const int32_t* taxon;            // [n_nodes] row of `counts` for a leaf, -1 for interior nodes
    const int32_t* n_rows;           // [n_nodes] factor rows s = 0..n_rows-1: M + 1, or R + 1 under the root
    const SlotParamLM* slots;        // [batch][n_nodes] the branch's parameters under the family's (lambdas, mus)
    const int64_t* col;              // [batch] the family's column in `counts`
    const int32_t* counts;           // [taxon][counts_ld]
    int64_t counts_ld;
    const double* err;               // [(M+1)][n_dev] or nullptr
    int32_t n_dev, M, ld, n_nodes;
    double* factors;                 // [batch][n_nodes][ld]
};

// one level of branches for `batch` listed families: grid (batch, n_level_nodes), one wave each; n = matrix order
hipError_t launch_family_lambda_lm(const FamLamArgsLM& a, int n, int64_t batch, int n_level_nodes, hipStream_t stream);

}  // namespace cafe
