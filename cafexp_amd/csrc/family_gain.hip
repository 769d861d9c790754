// cafe_score_per_family_gain: the per-family path under a gene gain rate.  Every other model of the library has size 0
// absorbing -- row 0 of every matrix is e_0 -- so a family that is absent in an ancestor and present later has likelihood 0
// whatever the rates.  With a gain rate nu (n -> n+1 at rate n lambda + nu, n -> n-1 at rate n mu: Kendall's birth-death-
// immigration process, the gain-loss-duplication model) a lineage count of 0 is left again.  The transition law from size s is
// the s-fold convolution of the single-lineage law p1 (bd_row.h, unchanged, the same alpha and beta) with the law of the
// immigrants' descendants, so the row recurrence is the one the per-family kernel runs already and only row 0 changes
// (family_gain_kernel.h).  The root may be absent too: root sizes run over 0..R,
//     t_0 = log L_0 + log(root_absent),   t_j = log L_j + log1p(-root_absent) + log (double)(float)prior_j  (j >= 1),
// under the max rule or the sum rule with the lane order and the fold tree of family_lambda.hip's root kernels; with
// root_absent = 0 the size-0 term is -inf and changes no bit.  The host frame is family_frame.h's.
#include "family_frame.h"
#include "family_gain_kernel.h"

namespace cafe {
namespace {

struct FamRootGainArgs {
    FamRootArgs f;
    double log_absent, log_present;  // log(root_absent), log1p(-root_absent)
};

// t_0 of a family: the root's children at parent size 0
__device__ __forceinline__ double gain_root_t0(const FamRootGainArgs& a, const double* __restrict__ fac_b) {
    double L = 1.0;
    for (int k = 0; k < a.f.n_root_children; ++k) L *= fac_b[(int64_t)a.f.root_children[k] * a.f.ld];
    return log(L) + a.log_absent;
}

// family_root_kernel over root sizes 0..R: lane 0 takes the size-0 term behind its own sizes
__global__ __launch_bounds__(64) void family_gain_root_kernel(const FamRootGainArgs a) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* __restrict__ fac_b = a.f.factors + b * a.f.n_nodes * a.f.ld;
    double best = -__builtin_huge_val();
    for (int j = lane; j < a.f.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.f.n_root_children; ++k) L *= fac_b[(int64_t)a.f.root_children[k] * a.f.ld + j + 1];
        const double full = log(L) + a.log_present + a.f.log_prior[j];
        if (j == 0 || full > best) best = full;
    }
    if (lane == 0) {
        const double t0 = gain_root_t0(a, fac_b);
        if (t0 > best) best = t0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_down(best, d);
        if (o > best) best = o;
    }
    if (lane == 0) a.f.out[b] = best;
}

// family_root_sum_kernel over root sizes 0..R: lane 0 adds the size-0 term in front of its own sizes
__global__ __launch_bounds__(64) void family_gain_root_sum_kernel(const FamRootGainArgs a) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* __restrict__ fac_b = a.f.factors + b * a.f.n_nodes * a.f.ld;
    const double ninf = -__builtin_huge_val();
    const double t0 = lane == 0 ? gain_root_t0(a, fac_b) : ninf;
    double m = ninf;
    for (int j = lane; j < a.f.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.f.n_root_children; ++k) L *= fac_b[(int64_t)a.f.root_children[k] * a.f.ld + j + 1];
        const double t = log(L) + a.log_present + a.f.log_prior[j];
        if (t > m) m = t;
    }
    if (t0 > m) m = t0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                // (butterfly: every lane ends with the maximum)
        const double o = __shfl_xor(m, d);
        if (o > m) m = o;
    }
    double s = t0 == ninf ? 0.0 : exp(t0 - m);
    for (int j = lane; j < a.f.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.f.n_root_children; ++k) L *= fac_b[(int64_t)a.f.root_children[k] * a.f.ld + j + 1];
        const double t = log(L) + a.log_present + a.f.log_prior[j];
        s += t == ninf ? 0.0 : exp(t - m);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
    if (lane == 0) a.f.out[b] = m + log(s);
}

bool beyond_long(double rate) { return !(rate * 1000000000 < 9.0e18); }

hipError_t launch_root(bool sum_rule, const FamRootArgs& ra, double root_absent, int64_t nb, hipStream_t s) {
    FamRootGainArgs ga{ra, std::log(root_absent), std::log1p(-root_absent)};
    (void)hipGetLastError();
    if (sum_rule) hipLaunchKernelGGL(family_gain_root_sum_kernel, dim3((unsigned)nb), dim3(64), 0, s, ga);
    else hipLaunchKernelGGL(family_gain_root_kernel, dim3((unsigned)nb), dim3(64), 0, s, ga);
    return hipGetLastError();
}

}  // namespace

int gain_rates_check(cafe_ctx* c, const char* who, int64_t n, const double* nus, double root_absent) {
    if (!(root_absent >= 0 && root_absent <= 1)) { set_err(c, "%s: root_absent %g outside [0, 1]", who, root_absent); return CAFE_ERR_ARGUMENT; }
    if (n > 0 && !nus) { set_err(c, "%s: nus are required", who); return CAFE_ERR_ARGUMENT; }
    for (int64_t i = 0; i < n * c->n_lambdas; ++i)
        if (!(nus[i] >= 0)) { set_err(c, "%s: gain rate %g of entry %lld is negative or NaN", who, nus[i], (long long)(i / c->n_lambdas)); return CAFE_ERR_ARGUMENT; }
    return CAFE_OK;
}
SlotParamGain gain_branch_slot(const cafe_ctx* c, int u, const double* lam, const double* mus, const double* nus) {
    const int i = c->lam_idx[u];
    const double l = lam[i], m = mus ? mus[i] : l, nu = nus[i];
    if (beyond_long(l) || beyond_long(m) || beyond_long(nu)) return slot_param_gain(0, 0, nu > 0 ? 1 : 0, 0, true);
    return slot_param_gain(quantize_lambda(l), quantize_lambda(m), quantize_lambda(nu), quantize_time(c->blen[u]));
}
hipError_t launch_family_gain(const FamLamArgs<SlotParamGain>& a, int n, int64_t batch, int n_level_nodes, hipStream_t stream) {
    if (batch <= 0 || n_level_nodes <= 0) return hipSuccess;
    if (n > bd_matrix_max_order() || n > a.ld || batch > 0x7fffffff || n_level_nodes > 65535) return hipErrorInvalidValue;
    dim3 grid((unsigned)batch, (unsigned)n_level_nodes), block(64);
    return for_lane_width(n, [&](auto e) {
        (void)hipGetLastError();
        hipLaunchKernelGGL((family_gain_kernel<decltype(e)::value>), grid, block, 0, stream, a);
        return hipGetLastError();
    });
}
hipError_t gain_root_sum(const FamRootArgs& ra, double root_absent, int64_t nb, hipStream_t s) { return launch_root(true, ra, root_absent, nb, s); }

namespace {

struct GainRates {
    using Slot = SlotParamGain;
    static constexpr const char* entry = "cafe_score_per_family_gain";
    static constexpr bool reads_context_rates = false;
    static constexpr bool absent_ok = true;
    double root_absent;

    static bool rates_ok(int L, const double* mus, const double*) { return death_rates_ok(L, mus); }      // (nus: checked for the whole call)
    static Slot slot(const cafe_ctx* c, int u, const double* lam, const double* mus, const double* nus) { return gain_branch_slot(c, u, lam, mus, nus); }
    static hipError_t branches(const FamLamArgs<Slot>& a, int n, int64_t nb, int nodes, hipStream_t s) { return launch_family_gain(a, n, nb, nodes, s); }
    hipError_t root(const cafe_ctx* c, const FamRootArgs& ra, int64_t nb, hipStream_t s) const { return launch_root(c->root_rule == CAFE_ROOT_SUM, ra, root_absent, nb, s); }
};

int score_per_family_gain_impl(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                               const double* nus, double root_absent, double* family_lnl) {
    if (const int rc = gain_rates_check(c, GainRates::entry, n, nus, root_absent)) return rc;
    return per_family_frame(GainRates{root_absent}, c, pr, n, family, lambdas, mus, nus, family_lnl);
}

}  // namespace
}  // namespace cafe

int cafe_score_per_family_gain(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                               const double* nus, double root_absent, double* family_lnl) {
    const int rc = cafe::guarded(ctx, "cafe_score_per_family_gain",
                                 [&] { return cafe::score_per_family_gain_impl(ctx, params, n, family, lambdas, mus, nus, root_absent, family_lnl); });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

int cafe_bd_gain_row0(double lambda, double mu, double nu, double t, int32_t n, double* out, double out_r[1]) {
    using namespace cafe;
    if (n < 0 || (n > 0 && !out) || !(lambda >= 0) || !(mu >= 0) || !(nu >= 0) || !(t >= 0)) return CAFE_ERR_ARGUMENT;
    if (beyond_long(lambda) || beyond_long(mu) || beyond_long(nu)) return CAFE_ERR_ARGUMENT;
    const SlotParamGain g = slot_param_gain(quantize_lambda(lambda), quantize_lambda(mu), quantize_lambda(nu), quantize_time(t));
    for (int32_t k = 0; k < n; ++k) out[k] = g.row0 == kGainRow0Unit ? (k == 0 ? 1.0 : 0.0) : std::exp(gain_row0_log(g, k));
    if (out_r) out_r[0] = quantize_lambda(nu) == 0 ? 0.0 : quantize_lambda(lambda) == 0 ? __builtin_huge_val() : g.r;
    return CAFE_OK;
}
