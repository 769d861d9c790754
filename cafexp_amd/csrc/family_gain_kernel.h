// The per-family branch kernel under a gene GAIN rate nu (family_gain.hip has the model): the linear birth-death process with
// immigration, n -> n+1 at rate n lambda + nu, n -> n-1 at rate n mu.  A lineage's own descendants follow the single-lineage law
// p1 of bd_row.h as before, so row s of P is still row s-1 convolved with p1 and the row step is bd_row_step as it is.  What
// changes is ROW 0: the descendants of the immigrants of a branch are negative binomial,
//     P[0][k] = C(r+k-1, k) (1-beta)^r beta^k,   r = nu / lambda,
// and for lambda = 0 (r -> inf, beta -> 0) Poisson with mean m = nu (1 - exp(-mu t)) / mu (nu t at mu = 0).  nu = 0 is e_0.
//
// One formula for the host helper (cafe_bd_gain_row0), the slot and the kernel: gain_row0_log gives log P[0][k] at one column,
// and along the columns P[0][k] = P[0][k-1] (ra + rb (k-1)) / k with (ra, rb) = (beta r, beta), or (m, 0) for Poisson.  A lane
// evaluates the logarithm at ONE of its E columns -- the last one while the law still rises into it, the first one otherwise,
// so that it starts from the largest value it owns up to the one lane that holds the mode -- and runs the ratio from there: an
// underflow can then only lose what lies below the lane's own start.
#pragma once

#include "family_lambda_kernel.h"

namespace cafe {

enum GainRow0 : int32_t {
    kGainRow0Unit = 0,               // e_0: nu = 0, or no time, or no immigrant can arrive
    kGainRow0Lgamma = 1,             // negative binomial, r < kGainStirlingFrom: through lgamma(r + k)
    kGainRow0Stirling = 2,           // negative binomial, larger r: lgamma(r + k) - lgamma(r) from Stirling's series, without the cancellation
    kGainRow0Poisson = 3,            // lambda = 0
};
constexpr double kGainStirlingFrom = 256.0;            // the series' first dropped term, 1 / (1680 x^7), is below 1e-20 from here on

// Per transition matrix of the gain kernel: SlotParamLM's members with their meaning, and what row 0 needs.
struct SlotParamGain {
    static constexpr bool two_rates = true;
    double alpha;
    double beta;
    double q;
    double r;                        // nu / lambda (negative binomial only)
    double lognorm;                  // lgamma: r log(1-beta) - lgamma(r); Stirling: r log(1-beta); Poisson: -m
    double logb;                     // log beta; Poisson: log m
    double ra, rb;                   // P[0][k] / P[0][k-1] = (ra + rb (k-1)) / k
    int32_t zero;
    int32_t row0;                    // GainRow0
};
__host__ __device__ inline double slot_tail(const SlotParamGain& sp) { return sp.beta; }
__host__ __device__ inline double slot_q(const SlotParamGain& sp) { return sp.q; }

// log P[0][k] for row0 != kGainRow0Unit
__host__ __device__ inline double gain_row0_log(const SlotParamGain& g, int k) {
    const double x = (double)k, lf = lgamma(x + 1.0);
    if (g.row0 == kGainRow0Poisson) return g.lognorm + x * g.logb - lf;
    if (g.row0 == kGainRow0Lgamma) return lgamma(g.r + x) - lf + g.lognorm + x * g.logb;
    // lgamma(r + k) - lgamma(r) = (r - 1/2) log1p(k / r) + k log(r + k) - k + S(r + k) - S(r), S(y) = 1/(12 y) - 1/(360 y^3) + 1/(1260 y^5);
    // k log(r + k) joins k log(beta): beta (r + k) stays of the order of the mean however large r is
    const double y = g.r + x, iy = 1.0 / y, ir = 1.0 / g.r, iy2 = iy * iy, ir2 = ir * ir;
    const double sy = iy * (1.0 / 12 - iy2 * (1.0 / 360 - iy2 * (1.0 / 1260))), sr = ir * (1.0 / 12 - ir2 * (1.0 / 360 - ir2 * (1.0 / 1260)));
    return (g.r - 0.5) * log1p(x / g.r) - x + x * log(g.beta * y) + (sy - sr) - lf + g.lognorm;
}

// The slot of the quantized key (lambda, mu, nu, t), all three rates quantized like a lambda.  beyond: a rate * 1e9 that does
// not fit a long (the caller's test) -- the saturated branch; with nu > 0 its row 0 is all zero (the mass has left every size).
inline SlotParamGain slot_param_gain(long lq, long mq, long nq, long tq, bool beyond = false) {
    SlotParamGain g{};
    g.row0 = kGainRow0Unit;
    if (beyond) {
        g.alpha = 1.0; g.beta = 1.0; g.q = 0.0; g.zero = 1;
        if (nq != 0) { g.row0 = kGainRow0Poisson; g.lognorm = -__builtin_huge_val(); }
        return g;
    }
    const SlotParamLM sp = slot_param_lm(lq, mq, tq);
    g.alpha = sp.alpha; g.beta = sp.beta; g.q = sp.q; g.zero = sp.zero;
    const double lambda = double(lq) / 1000000000.0, mu = double(mq) / 1000000000.0, nu = double(nq) / 1000000000.0, t = double(tq) / 1000.0;
    if (nq == 0) return g;
    if (lq == 0) {
        const double m = mq == 0 ? nu * t : nu * (-expm1(-mu * t)) / mu;
        if (!(m > 0)) return g;
        g.row0 = kGainRow0Poisson; g.lognorm = -m; g.logb = log(m); g.ra = m; g.rb = 0.0;
        return g;
    }
    if (!(g.beta > 0)) return g;
    g.r = nu / lambda;
    g.logb = log(g.beta); g.ra = g.beta * g.r; g.rb = g.beta;
    g.lognorm = g.r * log1p(-g.beta);
    g.row0 = g.r < kGainStirlingFrom ? kGainRow0Lgamma : kGainRow0Stirling;
    if (g.row0 == kGainRow0Lgamma) g.lognorm -= lgamma(g.r);
    return g;
}

// p[i] = P[0][c0 + i]
template <int E>
__device__ __forceinline__ void gain_row0(const SlotParamGain& g, int c0, double (&p)[E]) {
    if (g.row0 == kGainRow0Unit) {                     // the bits of family_lambda_kernel's start, not 0 * inf
#pragma unroll
        for (int i = 0; i < E; ++i) p[i] = (c0 + i == 0) ? 1.0 : 0.0;
        return;
    }
    const int last = c0 + E - 1;
    if (fma(g.rb, (double)(last - 1), g.ra) >= (double)last) {         // P[0][last] >= P[0][last - 1]: the law rises through the lane
        p[E - 1] = exp(gain_row0_log(g, last));
#pragma unroll
        for (int i = E - 1; i >= 1; --i) {
            const double k = (double)(c0 + i);
            p[i - 1] = p[i] * (k / fma(g.rb, k - 1.0, g.ra));
        }
    } else {
        p[0] = exp(gain_row0_log(g, c0));
#pragma unroll
        for (int i = 1; i < E; ++i) {
            const double k = (double)(c0 + i);
            p[i] = p[i - 1] * (fma(g.rb, k - 1.0, g.ra) / k);
        }
    }
}

// family_lambda_kernel's mapping, vector load, row step and parked dot product.  New: the recurrence starts from gain_row0, so
// the r = 0 row of the factor is sum_c P[0][c] v[c]; a saturated key writes that row and zeros below it; col[b] < 0 is
// CAFE_FAMILY_ABSENT, every leaf count 0.
template <int E>
__global__ __launch_bounds__(64) void family_gain_kernel(const FamLamArgs<SlotParamGain> a) {
    __shared__ double part[kPartRows * kPartLd];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int u = a.nodes[blockIdx.y];
    const SlotParamGain sp = a.slots[b * a.n_nodes + u];
    double* __restrict__ fac_b = a.factors + b * a.n_nodes * a.ld;
    double* __restrict__ out = fac_b + (int64_t)u * a.ld;
    const int c0 = lane * E;                           // owned columns c0 .. c0+E-1 of the current row
    const int n_rows = a.n_rows[u];

    const int tx = a.taxon[u];
    int x = 0;
    if (tx >= 0) {
        const int64_t col = a.col[b];
        if (col >= 0) x = a.counts[(int64_t)tx * a.counts_ld + col];
        if (count_is_missing(x)) {                     // a missing cell: the factor is exactly 1.0 for every parent size (cafe_kernels.h)
            for (int r = lane; r < n_rows; r += 64) out[r] = leaf_factor_or_one(x, 0.0);
            return;                                    // (block-uniform: the block is one (family, branch))
        }
    }

    double p[E];                                       // P[row][c0 + i]; columns past the matrix hold values in [0,1] that meet v = 0
    gain_row0<E>(sp, c0, p);

    double v[E];                                       // the child's likelihoods of sizes c0 .. c0+E-1 (0 past M)
    if (tx >= 0) {
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
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (c0 + i <= a.M) ? 1.0 : 0.0;
        for (int k = a.child_off[u]; k < a.child_off[u + 1]; ++k) {
            const double* __restrict__ f = fac_b + (int64_t)a.child_idx[k] * a.ld;
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (c0 + i <= a.M) v[i] *= f[c0 + i];
        }
    }

    const int n_run = sp.zero ? 1 : n_rows;            // saturated / degenerate: row 0 alone is run, rows s >= 1 are 0
    for (int r = 1 + lane; sp.zero && r < n_rows; r += 64) out[r] = 0.0;

    BdRowConsts<E, true> rc;
    rc.init(sp.alpha, sp.beta, sp.q, lane);
    for (int r = 0; r < n_run; ++r) {
        if (r > 0) bd_row_step<E, false>(rc, nullptr, 0.0, lane, p);
        double d = p[0] * v[0];
#pragma unroll
        for (int i = 1; i < E; ++i) d = fma(p[i], v[i], d);
        part[(r & (kPartRows - 1)) * kPartLd + lane] = d;
        if ((r & (kPartRows - 1)) == kPartRows - 1 || r == n_run - 1) {
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

// one level of branches for `batch` listed families: grid (batch, n_level_nodes), one wave each; n = matrix order.  Defined in
// family_gain.hip, so that the kernels are instantiated in that translation unit and nowhere else.
hipError_t launch_family_gain(const FamLamArgs<SlotParamGain>& a, int n, int64_t batch, int n_level_nodes, hipStream_t stream);

}  // namespace cafe
