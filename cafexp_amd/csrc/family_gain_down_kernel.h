// The DOWN pass of the per-family gain path (family_gain_posterior.hip has the entry): the posterior of every node's size given
// the family's counts.  family_gain_kernel (the up pass) leaves factor_v[s] = sum_c P_v[s][c] L_v[c] of every branch.  What the
// rest of the tree says about node u's size is
//     outside_u[c] = sum_s w[s] P_u[s][c],      w[s] = outside_p[s] * prod_{siblings v != u} factor_v[s]      (p = parent of u),
// with outside_root = the root mass, and posterior_u[c] = outside_u[c] L_u[c] / Z.  P_u is never stored: the wave runs the row
// recurrence the up pass runs -- gain_row0, then bd_row_step -- and where the up kernel takes a dot product of the row with L_u
// it adds w[s] times the row into an accumulator, acc[i] = fma(w[s], p[i], acc[i]): no LDS turn, no reduction inside the row
// loop, one wave-uniform weight per row.  The layout is the up kernel's: one wave per (family, branch), lane l owns columns
// l E .. l E + E - 1, the widths of for_lane_width, grid (batch, branches of one DEPTH) -- a branch is ready when its parent's
// outside vector is, so the launches go by depth from the root, which is not the up pass's level order reversed.
//
// Registers: p, acc, the step's h and the powers of beta are live in the loop, as p, v, h and the powers are in the up kernel.
// L_u is needed in front of the loop (p_gain reads row 0 against it) and behind it; it is formed twice, the second time from
// offsets the compiler cannot prove equal to the first, so that it is not kept across the loop.
#pragma once

#include "family_frame.h"
#include "family_gain_kernel.h"

namespace cafe {

struct FamGainDownArgs {
    FamLamArgs<SlotParamGain> f;     // the up pass's tables and factors; nodes: the branches of this depth
    const int32_t* parent;           // [n_nodes]
    const double* lnl;               // [batch] the root kernel's sum-rule lnL: Z = exp(lnl)
    double* outside;                 // [batch][n_nodes][ld]
    double* p_absent;                // [batch][n_nodes], and mean, p_gain, p_loss
    double* mean;
    double* p_gain;
    double* p_loss;
    double* posterior;               // nullptr or [batch][n_nodes][N]
    int32_t N;                       // cafe_matrix_size
};

struct FamGainDownRootArgs {
    FamGainDownArgs d;
    const int32_t* root_children;
    const double* mass;              // [R + 1] root_absent, (1 - root_absent) (double)(float)prior[j - 1]
    int32_t n_root_children, R, root;
};

__device__ __forceinline__ double gain_wave_sum(double s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

// L_u[c0 + i]: the up kernel's v.  x: the leaf's count (missing: 1 up to M).  z: an offset of 0 the compiler does not know.
template <int E>
__device__ __forceinline__ void gain_down_likelihood(const FamLamArgs<SlotParamGain>& a, const double* __restrict__ fac_b, int u, int tx, int x, int c0, int z,
                                                     double (&v)[E]) {
    if (tx >= 0) {
        if (count_is_missing(x)) {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = (c0 + i <= a.M + z) ? 1.0 : 0.0;
        } else if (a.err) {
            const int lo = x - (a.n_dev - 1) / 2 + z;  // taps outside [0, M] are dropped
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int c = c0 + i, t = c - lo;
                v[i] = (t >= 0 && t < a.n_dev && c <= a.M) ? a.err[(int64_t)x * a.n_dev + t] : 0.0;
            }
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = (c0 + i == x + z) ? 1.0 : 0.0;
        }
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = (c0 + i <= a.M) ? 1.0 : 0.0;
        for (int k = a.child_off[u]; k < a.child_off[u + 1]; ++k) {
            const double* __restrict__ f = fac_b + (int64_t)a.child_idx[k] * a.ld + z;
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (c0 + i <= a.M) v[i] *= f[c0 + i];
        }
    }
}

template <int E>
__global__ __launch_bounds__(64) void family_gain_down_kernel(const FamGainDownArgs a) {
    __shared__ double w[64 * E];                       // n_rows <= matrix order <= 64 E
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int u = a.f.nodes[blockIdx.y];
    const int nn = a.f.n_nodes, ld = a.f.ld, M = a.f.M;
    const SlotParamGain sp = a.f.slots[b * nn + u];
    const double* __restrict__ fac_b = a.f.factors + b * nn * ld;
    double* __restrict__ out_b = a.outside + b * nn * ld;
    const int c0 = lane * E;
    const int n_rows = a.f.n_rows[u];
    const int par = a.parent[u];
    const double Z = exp(a.lnl[b]);

    for (int s = lane; s < n_rows; s += 64) {          // the weights: what the parent's outside and the siblings say of parent size s
        double x = out_b[(int64_t)par * ld + s];
        for (int k = a.f.child_off[par]; k < a.f.child_off[par + 1]; ++k) {
            const int sib = a.f.child_idx[k];
            if (sib != u) x *= fac_b[(int64_t)sib * ld + s];
        }
        w[s] = x;
    }
    __syncthreads();                                   // one wave per block: orders the LDS writes before the uniform reads

    const int tx = a.f.taxon[u];
    int x = 0;
    if (tx >= 0) {
        const int64_t col = a.f.col[b];
        if (col >= 0) x = a.f.counts[(int64_t)tx * a.f.counts_ld + col];
    }
    const bool missing = tx >= 0 && count_is_missing(x);

    double p[E];                                       // P[row][c0 + i]
    gain_row0<E>(sp, c0, p);
    const double w0 = w[0];

    double g;                                          // sum_{c >= 1} P[0][c] L_u[c]
    if (missing) {                                     // the factor of a missing cell is 1.0, the untruncated row sum: so is this
        g = sp.row0 == kGainRow0Unit ? 0.0 : -expm1(gain_row0_log(sp, 0));
    } else {
        double v[E];
        gain_down_likelihood<E>(a.f, fac_b, u, tx, x, c0, 0, v);
        g = 0.0;
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (c0 + i >= 1) g = fma(p[i], v[i], g);
        g = gain_wave_sum(g);
    }

    double acc[E];
#pragma unroll
    for (int i = 0; i < E; ++i) acc[i] = w0 * p[i];
    double loss = 0.0;                                 // lane 0: sum_{s >= 1} w[s] P[s][0]

    const int n_run = sp.zero ? 1 : n_rows;            // saturated / degenerate: rows s >= 1 are 0
    BdRowConsts<E, true> rc;
    rc.init(sp.alpha, sp.beta, sp.q, lane);
    for (int r = 1; r < n_run; ++r) {
        const double wr = w[r];
        bd_row_step<E, false>(rc, nullptr, 0.0, lane, p);
#pragma unroll
        for (int i = 0; i < E; ++i) acc[i] = fma(wr, p[i], acc[i]);
        loss = fma(wr, p[0], loss);
    }

    if (a.f.child_off[u + 1] > a.f.child_off[u]) {     // outside_u for the node's children
        double* __restrict__ o = out_b + (int64_t)u * ld;
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (c0 + i <= M) o[c0 + i] = acc[i];
    }

    int z = 0;
    asm volatile("" : "+v"(z));
    double v[E];
    gain_down_likelihood<E>(a.f, fac_b, u, tx, x, c0, z, v);
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        acc[i] = (c0 + i <= M) ? acc[i] * v[i] / Z : 0.0;
        m = fma((double)(c0 + i), acc[i], m);
    }
    m = gain_wave_sum(m);
    const int64_t o = b * nn + u;
    if (lane == 0) {
        a.p_absent[o] = acc[0];
        a.mean[o] = m;
        a.p_gain[o] = w0 * g / Z;
        a.p_loss[o] = v[0] * loss / Z;
    }
    if (a.posterior) {
        double* __restrict__ po = a.posterior + o * a.N;
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (c0 + i < a.N) po[c0 + i] = acc[i];
    }
}

// The root: its outside vector is the root mass (what the branches under it read), its own posterior the mass times the product
// of its children's factors.  One wave per family, in front of the down launches.
__global__ __launch_bounds__(64) void family_gain_down_root_kernel(const FamGainDownRootArgs a) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int nn = a.d.f.n_nodes, ld = a.d.f.ld;
    const double* __restrict__ fac_b = a.d.f.factors + b * nn * ld;
    double* __restrict__ o = a.d.outside + (b * nn + a.root) * ld;
    const double Z = exp(a.d.lnl[b]);
    const int64_t at = b * nn + a.root;
    double m = 0.0;
    for (int s = lane; s < a.d.N; s += 64) {
        double post = 0.0;
        if (s <= a.R) {
            const double mass = a.mass[s];
            o[s] = mass;
            double L = mass;
            for (int k = 0; k < a.n_root_children; ++k) L *= fac_b[(int64_t)a.root_children[k] * ld + s];
            post = L / Z;
            m = fma((double)s, post, m);
            if (s == 0) a.d.p_absent[at] = post;
        }
        if (a.d.posterior) a.d.posterior[at * a.d.N + s] = post;
    }
    m = gain_wave_sum(m);
    if (lane == 0) {
        a.d.mean[at] = m;
        a.d.p_gain[at] = __builtin_nan("");
        a.d.p_loss[at] = __builtin_nan("");
    }
}

// the branches of one depth for `batch` listed families: grid (batch, n_depth_nodes), one wave each; n = matrix order
inline hipError_t launch_family_gain_down(const FamGainDownArgs& a, int n, int64_t batch, int n_depth_nodes, hipStream_t stream) {
    if (batch <= 0 || n_depth_nodes <= 0) return hipSuccess;
    if (n > bd_matrix_max_order() || n > a.f.ld || n != a.N || batch > 0x7fffffff || n_depth_nodes > 65535) return hipErrorInvalidValue;
    dim3 grid((unsigned)batch, (unsigned)n_depth_nodes), block(64);
    return for_lane_width(n, [&](auto e) {
        (void)hipGetLastError();
        hipLaunchKernelGGL((family_gain_down_kernel<decltype(e)::value>), grid, block, 0, stream, a);
        return hipGetLastError();
    });
}

}  // namespace cafe
