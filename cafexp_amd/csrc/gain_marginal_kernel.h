// cafe_gain_marginal_dense: the kernels of its down pass.  Included by gain_dense.hip inside its namespace, behind the kernels of
// cafe_gain_posterior_dense, whose tile constants, op tables (GainNodeOp, GainOutArgs) and helpers (gain_dense_fold4,
// gain_dense_shifted) it uses.
//
// The report wants, per node, mean / mode / interval of the posterior of its size and, per branch, the joint
//     J_u[s][c] = w_u[s] P_u[s][c] B_u[c] / Z        (s the parent's size, c the node's)
// split at the diagonal: p_increase = sum_{c > s} J, p_decrease = sum_{c < s} J, p_same = sum_{c = s} J.  Summed over s the
// joint is the node's posterior, outside_u[c] B_u[c] / Z, so ONE transposed GEMM whose contraction is cut at s = c gives both
// the outside panel the deeper depths need and the three sums; the summaries are then taken from outside and B without the
// posterior ever being stored.
//
//   split     gain_marginal_dense_split_kernel, in place of the transposed GEMM: grid (column tiles of 128, row tiles of 64
//             sizes c, interior non-root nodes of the depth).  One accumulator set, two phases over the 64 x 128 x 16 tile, the
//             two LDS buffer pairs, v_mfma_f64_16x16x4 and the XOR-swizzled transposing A staging of gain_dense_tile:
//               phase 1  s in [0, min(nk, r0 + 64)) with s < c: the K tiles below r0 whole, the four K tiles r0 .. r0 + 63 with
//                        the A element zeroed where s >= c -- the comparison is made once, on the staging registers ra[], as
//                        the tile is loaded, never in the MFMA loop.  Epilogue: inc[col] = sum_c B[c] acc[c], and the tile is
//                        PARKED in the O panel (a thread re-reads only what it wrote itself).
//               phase 2  s in [r0, nk) with s > c on a zeroed accumulator: the same four K tiles masked the other way, the tiles
//                        from r0 + 64 on whole.  Epilogue: dec[col] = sum_c B[c] acc[c]; the diagonal P[c][c] w[c] element by
//                        element on the VALU, same[col] = sum_c B[c] P[c][c] w[c]; O = (parked + diagonal) + phase 2.
//             A row tile therefore issues 8 K tiles more than the plain transposed GEMM (4 straddling tiles, once per side).
//             The three sums of a column over the tile's rows: a lane adds its 16 rows in ascending order, the four 16-lane
//             groups that share the column meet by two cross-lane exchanges, (g0 + g1) + (g2 + g3), and lane group 0 stores
//             them into parts[node][row tile][3][ld].  No atomics; the summary kernel folds the row tiles in ascending order.
//   interior  64 columns per block, lanes along the family; the four waves take CONTIGUOUS quarters of the node's sizes, so the
//             CDF is an ordered prefix.  Pass 1: mean, first arg max and the quarter's total; the totals meet in LDS; pass 2
//             walks the quarter again from its prefix and finds the first size whose CDF reaches (1 - level) / 2 and
//             1 - (1 - level) / 2.  The CDF is that of the posterior values as they are, each already divided by Z: its total is
//             taken as 1, never renormalised, and a threshold the CDF does not reach gives the node's last size
//             (marginal.hip's rule).  Wave y < 3 folds the row tiles' partials of one of the three branch probabilities.
//   leaf      no GEMM: O at a tap c is the dot along the contiguous column Pt[c * ldp + s], s cut at c into three sums of
//             their own.  Without an error model the row is the observed count; with one, the posterior over the taps.
// Scaled (cafe_set_gain_scaling): the split kernel runs on the mantissas as it is, and every ratio against Z~ is shifted with
// ldexp by the exponents of w, B and the root, as gain_posterior_dense_interior does.
#pragma once

struct GainSplitArgs {
    const GainNodeOp* ops;           // the depth's interior nodes: the contraction is op.rows, the partials stand at parts + op.node * tiles * 3 * ld
    const double* mats;
    double* panels;
    double* parts;                   // [n_nodes][row tiles][3][ld]: increase, decrease, same
    int64_t ld;
    int32_t nr, ldp;                 // rows c = 0..nr-1 of the outside panel
};

// where phase 1 of row tile r0 ends: behind its straddling K tiles, or with the contraction (the host counts the flops by it)
__host__ __device__ inline int gain_marginal_phase1_end(int r0, int nk) {
    const int k_end = (nk + kGdKT - 1) / kGdKT * kGdKT;
    return r0 + kGdMT < k_end ? r0 + kGdMT : k_end;
}

// grid (column tiles, row tiles of M + 1, interior non-root nodes of the depth)
__global__ __launch_bounds__(256) void gain_marginal_dense_split_kernel(const GainSplitArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][kGdKT * kGdLdA];
    __shared__ __attribute__((aligned(16))) double Xs[2][kGdKT * kGdLdX];
    const GainNodeOp op = a.ops[blockIdx.z];
    const int r0 = blockIdx.y * kGdMT, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4, nr = a.nr, nk = op.rows;
    const int64_t c0 = (int64_t)blockIdx.x * kGdCols, ld = a.ld;
    const int k_end = (nk + kGdKT - 1) / kGdKT * kGdKT;
    const double* __restrict__ mat = a.mats + op.Pt;
    const double* __restrict__ W = a.panels + op.W + c0 + 32 * wave + l15;
    const double* __restrict__ B = a.panels + op.B + c0 + 32 * wave + l15;
    double* __restrict__ O = a.panels + op.outside + c0 + 32 * wave + l15;
    gd4 acc[4][2];
    double inc[2] = {0.0, 0.0}, dec[2] = {0.0, 0.0}, same[2] = {0.0, 0.0};

    gain_dense_tile<kGdAStored, +1>(As, Xs, mat, a.panels + op.W, r0, nr, 0, gain_marginal_phase1_end(r0, nk), nk, a.ldp, ld, c0, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + 16 * i + l4 + 4 * q;
            if (r >= nr) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                inc[j] = fma(B[(int64_t)r * ld + 16 * j], acc[i][j][q], inc[j]);
                O[(int64_t)r * ld + 16 * j] = acc[i][j][q];                 // parked: read back below by this thread alone
            }
        }

    gain_dense_tile<kGdAStored, -1>(As, Xs, mat, a.panels + op.W, r0, nr, r0, k_end, nk, a.ldp, ld, c0, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + 16 * i + l4 + 4 * q;
            if (r >= nr) continue;
            const double pd = r < nk ? mat[(int64_t)r * a.ldp + r] : 0.0;   // P[r][r]; past the parent's sizes there is no diagonal
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double b = B[(int64_t)r * ld + 16 * j];
                const double diag = r < nk ? pd * W[(int64_t)r * ld + 16 * j] : 0.0;
                dec[j] = fma(b, acc[i][j][q], dec[j]);
                same[j] = fma(b, diag, same[j]);
                O[(int64_t)r * ld + 16 * j] = (O[(int64_t)r * ld + 16 * j] + diag) + acc[i][j][q];
            }
        }

    double* __restrict__ part = a.parts + ((int64_t)op.node * gridDim.y + blockIdx.y) * 3 * ld + c0 + 32 * wave + l15;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double v[3] = {inc[j], dec[j], same[j]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] += __shfl_xor(v[k], 16);
            v[k] += __shfl_xor(v[k], 32);
            if (l4 == 0) part[(int64_t)k * ld + 16 * j] = v[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ summaries
// res is [4][n_nodes][ld]: mean, p_increase, p_decrease, p_same; ires [3][n_nodes][ld]: mode, lo, hi.  The op tables are the
// output kernels' (GainNodeOp); a.posterior is not read.
struct GainSummaryArgs {
    GainOutArgs o;
    const double* parts;             // the split kernel's partials
    int32_t* ires;
    double level;
    int32_t tiles;                   // row tiles of the split kernel
};

struct GainCdf {                     // the walk along a CDF: the first size at which it reaches either threshold
    double tlo, thi, cum;
    int lo, hi;
    __device__ __forceinline__ void step(int c, double p) {
        cum += p;
        if (lo < 0 && cum >= tlo) lo = c;
        if (hi < 0 && cum >= thi) hi = c;
    }
};

// grid (cols / 64, interior nodes of the depth), the root among them: its outside vector is `mass`, its three p's NaN
template <bool Scaled>
__device__ __forceinline__ void gain_marginal_interior(const GainSummaryArgs& a, double (*red)[64], int (*ired)[64], const int32_t* exps) {
    const GainNodeOp op = a.o.ops[blockIdx.y];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 64 + x, ld = a.o.ld;
    const bool root = op.W < 0;
    const double Z = exp(a.o.lnl[f]);
    int d = 0;
    if constexpr (Scaled)
        if (!root) d = exps[op.W / a.o.N + f] + exps[op.B / a.o.N + f] - exps[a.o.root_B / a.o.N + f];
    const double* __restrict__ B = a.o.panels + op.B + f;
    const double* __restrict__ O = a.o.panels + (root ? op.B : op.outside) + f;
    const int chunk = (op.n + 3) / 4, c_lo = min(op.n, y * chunk), c_hi = min(op.n, c_lo + chunk);
    auto post_at = [&](int c) { return gain_dense_shifted<Scaled>((root ? a.o.mass[c] : O[(int64_t)c * ld]) * B[(int64_t)c * ld] / Z, d); };

    double m = 0.0, best = -1.0, seg = 0.0;
    int arg = c_lo;
    for (int c = c_lo; c < c_hi; ++c) {
        const double post = post_at(c);
        m = fma((double)c, post, m);
        if (post > best) { best = post; arg = c; }
        seg += post;
    }
    m = gain_dense_fold4(red, x, y, m);
    red[y][x] = best;
    ired[y][x] = arg;
    __syncthreads();
    best = red[0][x];
    arg = ired[0][x];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (red[k][x] > best) { best = red[k][x]; arg = ired[k][x]; }      // strictly above: the first arg max
    __syncthreads();
    red[y][x] = seg;
    __syncthreads();
    GainCdf cdf{0.5 * (1.0 - a.level), 1.0 - 0.5 * (1.0 - a.level), 0.0, -1, -1};
    for (int k = 0; k < y; ++k) cdf.cum += red[k][x];  // the quarters below, in order
    for (int c = c_lo; c < c_hi; ++c) cdf.step(c, post_at(c));
    __syncthreads();
    ired[y][x] = cdf.lo;
    __syncthreads();
    int lo = -1;
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if (ired[k][x] >= 0) lo = ired[k][x];          // the lowest quarter that met the threshold
    __syncthreads();
    ired[y][x] = cdf.hi;
    __syncthreads();
    int hi = -1;
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if (ired[k][x] >= 0) hi = ired[k][x];

    const int64_t o = (int64_t)op.node * ld + f, plane = (int64_t)a.o.nn * ld;
    if (y < 3) {                                       // wave y: one of p_increase, p_decrease, p_same
        double s = 0.0;
        if (!root) {
            const double* __restrict__ part = a.parts + ((int64_t)op.node * a.tiles * 3 + y) * ld + f;
            for (int t = 0; t < a.tiles; ++t) s += part[(int64_t)t * 3 * ld];
        }
        a.o.res[o + (1 + y) * plane] = root ? __builtin_nan("") : gain_dense_shifted<Scaled>(s / Z, d);
    }
    if (y != 0) return;
    a.o.res[o] = m;
    a.ires[o] = arg;
    a.ires[o + plane] = lo < 0 ? op.n - 1 : lo;
    a.ires[o + 2 * plane] = hi < 0 ? op.n - 1 : hi;
}

__global__ __launch_bounds__(256) void gain_marginal_dense_interior_kernel(const GainSummaryArgs a) {
    __shared__ double red[4][64];
    __shared__ int ired[4][64];
    gain_marginal_interior<false>(a, red, ired, nullptr);
}

__global__ __launch_bounds__(256) void gain_marginal_scaled_interior_kernel(const GainSummaryArgs a, const int32_t* exps) {
    __shared__ double red[4][64];
    __shared__ int ired[4][64];
    gain_marginal_interior<true>(a, red, ired, exps);
}

// grid (cols / 64, leaves of the depth).  The four waves take a quarter of the parent's sizes each, as in
// gain_posterior_dense_leaf; the dot at a tap is cut into s < c, s = c and s > c.  A count past M made lnl -inf: nothing is read
// for it and the host keeps the entry's NaN / -1.  (The entry refuses a context with missing cells.)
template <bool Scaled>
__device__ __forceinline__ void gain_marginal_leaf(const GainSummaryArgs& a, double (*red)[64], const int32_t* exps) {
    const GainNodeOp op = a.o.ops[blockIdx.y];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 64 + x, ld = a.o.ld;
    const double Z = exp(a.o.lnl[f]);
    int d = 0;
    if constexpr (Scaled) d = exps[op.W / a.o.N + f] - exps[a.o.root_B / a.o.N + f];
    const int64_t col = a.o.col[f];
    const int cnt = col >= 0 ? a.o.counts[(int64_t)op.taxon * a.o.counts_ld + col] : 0;
    const bool in = cnt >= 0 && cnt <= a.o.M;
    const double* __restrict__ W = a.o.panels + op.W + f;
    const double* __restrict__ Pt = a.o.mats + op.Pt;
    const int chunk = (op.rows + 3) / 4, s_lo = y * chunk, s_hi = min(op.rows, s_lo + chunk);
    const bool err = a.o.err != nullptr;
    const int n_taps = err ? a.o.n_dev : 1, first = err ? cnt - (a.o.n_dev - 1) / 2 : cnt;

    double mean = 0.0, best = -1.0, inc = 0.0, dec = 0.0, same = 0.0;
    int arg = 0, last = 0;
    GainCdf cdf{0.5 * (1.0 - a.level), 1.0 - 0.5 * (1.0 - a.level), 0.0, -1, -1};
    for (int t = 0; t < n_taps; ++t) {                 // taps ascending; those outside [0, M] are dropped
        const int c = first + t;
        const bool ok = in && c >= 0 && c <= a.o.M;    // (uniform over the four waves of a column)
        double lt = 0.0, gt = 0.0;
        if (ok) {
            const double* __restrict__ pc = Pt + (int64_t)c * a.o.ldp;
            for (int s = s_lo; s < min(s_hi, c); ++s) lt = fma(W[(int64_t)s * ld], pc[s], lt);
            for (int s = max(s_lo, c + 1); s < s_hi; ++s) gt = fma(W[(int64_t)s * ld], pc[s], gt);
        }
        lt = gain_dense_fold4(red, x, y, lt);
        gt = gain_dense_fold4(red, x, y, gt);
        if (y != 0 || !ok) continue;
        const double eq = c < op.rows ? W[(int64_t)c * ld] * Pt[(int64_t)c * a.o.ldp + c] : 0.0;
        const double wt = err ? a.o.err[(int64_t)cnt * a.o.n_dev + t] : 1.0;
        const double post = gain_dense_shifted<Scaled>(((lt + eq) + gt) * wt / Z, d);
        inc = fma(wt, lt, inc);
        dec = fma(wt, gt, dec);
        same = fma(wt, eq, same);
        mean = fma((double)c, post, mean);
        if (post > best) { best = post; arg = c; }
        cdf.step(c, post);
        last = c;
    }
    if (y != 0) return;
    const int64_t o = (int64_t)op.node * ld + f, plane = (int64_t)a.o.nn * ld;
    a.o.res[o] = err ? mean : (double)cnt;             // without an error model the row is the observed count
    a.o.res[o + plane] = gain_dense_shifted<Scaled>(inc / Z, d);
    a.o.res[o + 2 * plane] = gain_dense_shifted<Scaled>(dec / Z, d);
    a.o.res[o + 3 * plane] = gain_dense_shifted<Scaled>(same / Z, d);
    a.ires[o] = err ? arg : cnt;
    a.ires[o + plane] = !err ? cnt : cdf.lo < 0 ? last : cdf.lo;
    a.ires[o + 2 * plane] = !err ? cnt : cdf.hi < 0 ? last : cdf.hi;
}

__global__ __launch_bounds__(256) void gain_marginal_dense_leaf_kernel(const GainSummaryArgs a) {
    __shared__ double red[4][64];
    gain_marginal_leaf<false>(a, red, nullptr);
}

__global__ __launch_bounds__(256) void gain_marginal_scaled_leaf_kernel(const GainSummaryArgs a, const int32_t* exps) {
    __shared__ double red[4][64];
    gain_marginal_leaf<true>(a, red, exps);
}
