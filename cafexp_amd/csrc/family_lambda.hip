// cafe_score_per_family: one scorer evaluation for a list of families, EACH WITH ITS OWN lambdas -- what the reference's
// lambda-per-family mode (-b; estimator::estimate_lambda_per_family, src/execute.cpp:104-128) asks of the scorer, one
// family at a time.
//
// With one lambda vector per family nothing of the scorer path applies: every family has its own transition matrices, a
// branch is a matrix-vector product and not a GEMM, and a matrix is used exactly once.  So no matrix is ever written:
//   branch kernel   ONE 64-lane wave per (listed family, branch).  The wave loads the child's likelihood vector v (a leaf:
//                   one-hot at the observed count, or the error-model taps around it; an interior node: the product of its
//                   children's factors, multiplied on load), runs K1's row recurrence (bd_row.h: a lane owns E consecutive
//                   columns of the row, DPP scan; the same quantized key, the same special cases) and after every row step
//                   forms factor[s] = sum_c P[s][c] v[c], c = 0..M.
//   the dot product The lane partials of a row must be summed across the wave, and that sum must not sit on the dependent
//                   chain of row steps (a row step IS the kernel's latency).  A lane parks its partial in LDS
//                   (part[row % 16][lane]) and goes on; every 16 rows the block is summed transposed -- lane (j, quarter)
//                   adds 16 partials of row j, two cross-lane adds fold the quarters -- and 16 lanes store 16 factors.
//                   16 rows and not 64: 8 KB of LDS per wave instead of 33 KB, so LDS never limits the waves per CU.
//   levels          Children first, ONE LAUNCH PER LEVEL over (families x branches of the level): the unit of work stays
//                   one wave whatever the tree's shape, a launch of the mammals table has >= 12 653 waves, and late in a
//                   search -- few unfinished families -- the branches of a level still spread over the chip, which one
//                   workgroup per family (a barrier per level, as many waves as the widest level) would not.
//   root kernel     one wave per family: L[j] = prod_children factor[j + 1], j = 0..R-1, then what K4 applies:
//                   max_j(log L_j + log (double)(float)prior_j) (base_model.cpp:95-102).
// Factors live in a workspace [listed family][node][ld] doubles.  The list is cut into batches that fit the context's
// workspace_limit (0 = automatic); a family's value depends on its counts and lambdas only, never on the cut.
// Every leaf branch runs all its rows (the reversibility short cut for a leaf without error model -- c row steps for a
// count c -- is not taken).  The host frame is family_frame.h's, shared with cafe_score_per_family_gain (family_gain.hip).
#include "family_frame.h"

namespace cafe {

// the branch kernel (family_lambda_kernel.h) for lambda = mu; family_lambda_lm.hip holds the two-rate instantiation
template hipError_t launch_family_lambda<SlotParam>(const FamLamArgs<SlotParam>&, int, int64_t, int, hipStream_t);

namespace {

// lnL_f = max_j(log L_j + log prior_j) (base_model.cpp:94-101), L_j = prod over the root's children of factor[j + 1]
__global__ __launch_bounds__(64) void family_root_kernel(const FamRootArgs a) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* __restrict__ fac_b = a.factors + b * a.n_nodes * a.ld;
    double best = -__builtin_huge_val();
    for (int j = lane; j < a.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.n_root_children; ++k) L *= fac_b[(int64_t)a.root_children[k] * a.ld + j + 1];
        const double full = log(L) + a.log_prior[j];
        if (j == 0 || full > best) best = full;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_down(best, d);
        if (o > best) best = o;
    }
    if (lane == 0) a.out[b] = best;
}

// ... and under CAFE_ROOT_SUM (cafe_set_root_rule) lnL_f = log sum_j L_j prior_j as K4's sum rule evaluates it: m = max_j t_j,
// t_j = log L_j + log prior_j, then m + log sum_j exp(t_j - m) -- a lane adds its rows j = lane, lane + 64, ... in ascending
// order, the lanes are folded by a fixed tree.  All t_j = -inf: -inf; a NaN term: NaN.  A kernel of its own: the max rule's
// code stays what it was.
__global__ __launch_bounds__(64) void family_root_sum_kernel(const FamRootArgs a) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* __restrict__ fac_b = a.factors + b * a.n_nodes * a.ld;
    const double ninf = -__builtin_huge_val();
    double m = ninf;
    for (int j = lane; j < a.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.n_root_children; ++k) L *= fac_b[(int64_t)a.root_children[k] * a.ld + j + 1];
        const double t = log(L) + a.log_prior[j];
        if (t > m) m = t;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                // (butterfly: every lane ends with the maximum)
        const double o = __shfl_xor(m, d);
        if (o > m) m = o;
    }
    double s = 0.0;
    for (int j = lane; j < a.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.n_root_children; ++k) L *= fac_b[(int64_t)a.root_children[k] * a.ld + j + 1];
        const double t = log(L) + a.log_prior[j];
        s += t == ninf ? 0.0 : exp(t - m);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
    if (lane == 0) a.out[b] = m + log(s);
}

// The branch above node u under one family's lambdas
SlotParam branch_param(const cafe_ctx* c, int u, const double* lam) {
    const double l = lam[c->lam_idx[u]];
    if (!(l * 1000000000 < 9.0e18)) {                  // beyond a long: saturated on any branch (lambdas are >= 0 and not NaN here)
        SlotParam sp{};
        sp.alpha = 1.0; sp.oma2 = 0.0; sp.zero = 1;
        return sp;
    }
    return slot_param(quantize_lambda(l), quantize_time(c->blen[u]));
}
// What the two entries differ in (family_frame.h): the slot type (the branch kernel's argument block and launcher follow from
// it) and how a family's rates become a branch's slot.  mus is null for the lambda = mu entry.  Both end in the root kernels above.
struct BirthDeathRoot {
    static constexpr bool absent_ok = false;
    hipError_t root(const cafe_ctx* c, const FamRootArgs& ra, int64_t nb, hipStream_t s) const {
        (void)hipGetLastError();
        if (c->root_rule == CAFE_ROOT_SUM) hipLaunchKernelGGL(family_root_sum_kernel, dim3((unsigned)nb), dim3(64), 0, s, ra);
        else hipLaunchKernelGGL(family_root_kernel, dim3((unsigned)nb), dim3(64), 0, s, ra);
        return hipGetLastError();
    }
};
struct EqualRates : BirthDeathRoot {
    using Slot = SlotParam;
    static constexpr const char* entry = "cafe_score_per_family";
    static constexpr bool reads_context_rates = true;  // lambda = mu is what it computes: refused while the context has death rates
    static bool rates_ok(int, const double*, const double*) { return true; }
    static Slot slot(const cafe_ctx* c, int u, const double* lam, const double*, const double*) { return branch_param(c, u, lam); }
    static hipError_t branches(const FamLamArgs<Slot>& a, int n, int64_t nb, int nodes, hipStream_t s) { return launch_family_lambda(a, n, nb, nodes, s); }
};
struct TwoRates : BirthDeathRoot {
    using Slot = SlotParamLM;
    static constexpr const char* entry = "cafe_score_per_family_lm";
    static constexpr bool reads_context_rates = false;
    static bool rates_ok(int L, const double* mus, const double*) { return death_rates_ok(L, mus); }
    static Slot slot(const cafe_ctx* c, int u, const double* lam, const double* mus, const double*) { return branch_param_lm(c, u, lam, mus); }
    static hipError_t branches(const FamLamArgs<Slot>& a, int n, int64_t nb, int nodes, hipStream_t s) { return launch_family_lambda(a, n, nb, nodes, s); }
};

}  // namespace

int score_per_family_impl(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, double* family_lnl) {
    return per_family_frame(EqualRates{}, c, pr, n, family, lambdas, nullptr, nullptr, family_lnl);
}
int score_per_family_lm_impl(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                             double* family_lnl) {
    if (n > 0 && !mus) { set_err(c, "cafe_score_per_family_lm: mus are required"); return CAFE_ERR_ARGUMENT; }
    return per_family_frame(TwoRates{}, c, pr, n, family, lambdas, mus, nullptr, family_lnl);
}

}  // namespace cafe

int cafe_score_per_family(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family, const double* lambdas, double* family_lnl) {
    const int rc = cafe::guarded(ctx, "cafe_score_per_family", [&] { return cafe::score_per_family_impl(ctx, params, n, family, lambdas, family_lnl); });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

int cafe_score_per_family_lm(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                             double* family_lnl) {
    const int rc = cafe::guarded(ctx, "cafe_score_per_family_lm", [&] { return cafe::score_per_family_lm_impl(ctx, params, n, family, lambdas, mus, family_lnl); });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}
