// cafe_gain_score_gradient: the kernels of its down pass.  Included by gain_dense.hip inside its namespace, behind the kernels of
// cafe_gain_posterior_dense, whose tile loop (gain_dense_tile), op table (GainNodeOp) and fold (gain_dense_fold4) it uses.
//
// The branch above v has the three parameters alpha, beta (cafe_bd_rates) and r = nu / lambda; row s of its matrix has the
// generating function G0 g^s, G0(z) = ((1 - beta) / (1 - beta z))^r, g(z) = (alpha + (1 - alpha - beta) z) / (1 - beta z).  With,
// along a row, H: y[j] = x[j] + beta y[j-1], S the shift by one, D = I - S and (Lambda x)[j] = sum_{k >= 1} (beta^k / k) x[j-k],
//     dP[s]/dalpha = s H D P[s-1]
//     dP[s]/dbeta  = -s (1 - alpha) H H S D P[s-1] - (r / (1 - beta)) H D P[s]
//     dP[s]/dr     = ln(1 - beta) P[s] + Lambda P[s]                                     (valid at r = 0)
// and all four operators are lower triangular, so the identities hold on the matrix cut at M.  With w = w_v,
// B = B_v, O = P^T w (the outside panel) and a SECOND outside panel O'[c] = sum_{s >= 1} s w[s] P[s-1][c]:
//     dZ/dalpha = O'^T (D^T H^T B)
//     dZ/dbeta  = -(1 - alpha) O'^T (D^T S^T H^T H^T B) - (r / (1 - beta)) O^T (D^T H^T B)
//     dZ/dr     = ln(1 - beta) Z + O^T (Lambda^T B),      (Lambda^T B)[c] = sum_{k > c} (beta^(k-c) / (k-c)) B[k]
//
//   outside2  O' by the transposed GEMM's tile with its right-hand side staged as X'[k] = (k + 1) w[k + 1]
//   toeplitz  O^T (Lambda^T B): a GEMM whose A is the strictly upper triangular Toeplitz matrix of L[j] = beta^j / j.  A is never
//             loaded: the staging registers are filled from the key's table of M + 1 doubles.  A row tile starts at its diagonal
//             K tile.  The product is not stored: the accumulators are multiplied by the O tile and summed over the tile's rows
//             (the split GEMM's lane order) into parts[node][row tile][ld]
//   interior  one thread per column: the anti-causal scans H^T B and H^T H^T B from M down to 0 (gradient_scan_kernel's), dotted
//             with O and O' on the way; the toeplitz partials folded in ascending tile order; three doubles per (node, column)
//   filter    per distinct LEAF key the three derivative matrices in the stored (k-major) form, thread s running the causal
//   lambda    recurrences along c (loads coalesced over s); the Lambda filter is a direct sum, 16 sizes c per thread
//   leaf      the posterior leaf kernel's gather over the three derivative matrices at the taps of the observed count
// Everything is divided by Z = exp(lnl).  No atomics: a value depends on the family's counts and the rates only.
#pragma once

struct GainGradArgs {
    const GainNodeOp* ops;           // the depth's interior nodes (O' of the k-th stands at o2 + k pan_stride), or its leaves
    const SlotParamGain* slots;      // [keys]
    const double* mats;
    double* panels;
    const double* ltab;              // [keys][ldl]: 0, beta, beta^2 / 2, .., beta^M / M, then zeros
    double* parts;                   // [n_nodes][tiles][ld]
    double* dmats;                   // [leaf keys][3][mat_stride]: d/dalpha, d/dbeta, d/dr of the matrix, stored as it is
    const int32_t* leaf_keys;        // [leaf keys] their keys
    const int32_t* dmat_of;          // [keys] the key's place among the leaf keys, -1: no leaf has it
    const double* lnl;               // [ld] the root kernel's sum-rule lnL
    double* res;                     // [3][n_nodes][ld]: d_alpha, d_beta, d_r
    const int64_t* col;
    const int32_t* counts;
    const double* err;
    int64_t counts_ld, ld, ncols, mat_stride, pan_stride, o2;
    int32_t nn, N, M, ldp, ldl, n_dev, tiles;
};

constexpr int kGgChunk = 16;         // sizes c per thread of the Lambda filter

// grid (column tiles, row tiles of M + 1, interior non-root nodes of the depth)
__global__ __launch_bounds__(256) void gain_gradient_outside2_kernel(const GainGradArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][kGdKT * kGdLdA];
    __shared__ __attribute__((aligned(16))) double Xs[2][kGdKT * kGdLdX];
    const GainNodeOp op = a.ops[blockIdx.z];
    const int r0 = blockIdx.y * kGdMT;
    const int64_t c0 = (int64_t)blockIdx.x * kGdCols;
    gd4 acc[4][2];
    gain_dense_tile<kGdAStored, 0, true>(As, Xs, a.mats + op.Pt, a.panels + op.W, r0, a.M + 1, 0, op.rows - 1, op.rows - 1, a.ldp, a.ld, c0, acc);
    gain_dense_tile_store(a.panels + a.o2 + (int64_t)blockIdx.z * a.pan_stride, r0, a.M + 1, a.ld, c0, acc);
}

// grid (column tiles, row tiles of M + 1, interior non-root nodes of the depth); after the depth's transposed GEMM
__global__ __launch_bounds__(256) void gain_gradient_toeplitz_kernel(const GainGradArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][kGdKT * kGdLdA];
    __shared__ __attribute__((aligned(16))) double Xs[2][kGdKT * kGdLdX];
    const GainNodeOp op = a.ops[blockIdx.z];
    const int r0 = blockIdx.y * kGdMT, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4, nr = a.M + 1;
    const int64_t c0 = (int64_t)blockIdx.x * kGdCols, ld = a.ld;
    const double* __restrict__ L = a.ltab + (op.Pt / a.mat_stride) * a.ldl;
    gd4 acc[4][2];
    gain_dense_tile<kGdAToeplitz, 0>(As, Xs, L, a.panels + op.B, r0, nr, r0, nr, nr, a.ldp, ld, c0, acc);
    const double* __restrict__ O = a.panels + op.outside + c0 + 32 * wave + l15;
    double t[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + 16 * i + l4 + 4 * q;
            if (r >= nr) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) t[j] = fma(O[(int64_t)r * ld + 16 * j], acc[i][j][q], t[j]);
        }
    double* __restrict__ part = a.parts + ((int64_t)op.node * a.tiles + blockIdx.y) * ld + c0 + 32 * wave + l15;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        t[j] += __shfl_xor(t[j], 16);
        t[j] += __shfl_xor(t[j], 32);
        if (l4 == 0) part[16 * j] = t[j];
    }
}

// grid (column blocks of 256, interior nodes of the depth), the root among them: NaN in its three.  Walked from M down:
// w1[j] = B[j] + beta w1[j+1], w2[j] = w1[j] + beta w2[j+1]; (D^T H^T B)[j] = w1[j] - w1[j+1], (D^T S^T H^T H^T B)[j] = w2[j+1] - w2[j+2].
// Eight rows of the three panels are loaded ahead of the recurrence that consumes them.
__global__ __launch_bounds__(256) void gain_gradient_interior_kernel(const GainGradArgs a) {
    const GainNodeOp op = a.ops[blockIdx.y];
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x, ld = a.ld;
    if (f >= a.ncols) return;
    const int64_t o = (int64_t)op.node * ld + f, plane = (int64_t)a.nn * ld;
    if (op.W < 0) {
        a.res[o] = a.res[o + plane] = a.res[o + 2 * plane] = __builtin_nan("");
        return;
    }
    const SlotParamGain sp = a.slots[op.Pt / a.mat_stride];
    const double beta = sp.beta;
    const double* __restrict__ B = a.panels + op.B + f;
    const double* __restrict__ O = a.panels + op.outside + f;
    const double* __restrict__ O2 = a.panels + a.o2 + (int64_t)blockIdx.y * a.pan_stride + f;
    double w1 = 0.0, w2 = 0.0, w2n = 0.0, sa = 0.0, sb = 0.0, sc = 0.0;    // w1[j+1], w2[j+1], w2[j+2]
    for (int j0 = a.M; j0 >= 0; j0 -= 8) {
        double b[8], x[8], x2[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool in = j0 - q >= 0;
            b[q] = in ? B[(int64_t)(j0 - q) * ld] : 0.0;
            x[q] = in ? O[(int64_t)(j0 - q) * ld] : 0.0;
            x2[q] = in ? O2[(int64_t)(j0 - q) * ld] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (j0 - q < 0) break;
            const double w1j = b[q] + beta * w1, d1 = w1j - w1, d2 = w2 - w2n;
            sa = fma(x2[q], d1, sa);
            sb = fma(x2[q], d2, sb);
            sc = fma(x[q], d1, sc);
            w2n = w2;
            w2 = w1j + beta * w2;
            w1 = w1j;
        }
    }
    double t = 0.0;
    const double* __restrict__ part = a.parts + (int64_t)op.node * a.tiles * ld + f;
    for (int k = 0; k < a.tiles; ++k) t += part[(int64_t)k * ld];
    const double Z = exp(a.lnl[f]);
    a.res[o] = sa / Z;
    a.res[o + plane] = (-(1.0 - sp.alpha) * sb - sp.r / (1.0 - beta) * sc) / Z;
    a.res[o + 2 * plane] = log1p(-beta) + t / Z;
}

// grid (blocks of 64 parent sizes s, leaf keys); thread s walks c = 0..M of rows s - 1 and s of the stored matrix:
// y = H D P[s-1], z = H y, u = H D P[s];  d/dalpha = s y[c],  d/dbeta = -s (1 - alpha) z[c-1] - (r / (1 - beta)) u[c]
__global__ __launch_bounds__(64) void gain_gradient_filter_kernel(const GainGradArgs a) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.N) return;
    const int key = a.leaf_keys[blockIdx.y];
    const SlotParamGain sp = a.slots[key];
    const double* __restrict__ Pt = a.mats + (int64_t)key * a.mat_stride + s;
    double* __restrict__ Da = a.dmats + (int64_t)blockIdx.y * 3 * a.mat_stride + s;
    double* __restrict__ Db = Da + a.mat_stride;
    const double beta = sp.beta, fs = (double)s, cz = fs * (1.0 - sp.alpha), cu = sp.r / (1.0 - beta);
    double xp = 0.0, pp = 0.0, y = 0.0, z = 0.0, u = 0.0;
#pragma unroll 4
    for (int c = 0; c <= a.M; ++c) {
        const double p = Pt[(int64_t)c * a.ldp], x = s > 0 ? Pt[(int64_t)c * a.ldp - 1] : 0.0;
        y = (x - xp) + beta * y;
        u = (p - pp) + beta * u;
        xp = x;
        pp = p;
        Da[(int64_t)c * a.ldp] = fs * y;
        Db[(int64_t)c * a.ldp] = -cz * z - cu * u;         // z still holds z[c-1]
        z = y + beta * z;
    }
}

// grid (blocks of 64 parent sizes s, chunks of 16 sizes c, leaf keys): d/dr [s][c] = ln(1 - beta) P[s][c] + sum_{j < c} L[c-j] P[s][j],
// j ascending; a value of the row is loaded once for the chunk's 16 sums.  (L is padded with zeros past M: the last chunk reads them.)
__global__ __launch_bounds__(64) void gain_gradient_lambda_kernel(const GainGradArgs a) {
    const int s = blockIdx.x * 64 + threadIdx.x, cc0 = blockIdx.y * kGgChunk;
    if (s >= a.N) return;
    const int key = a.leaf_keys[blockIdx.z];
    const double* __restrict__ Pt = a.mats + (int64_t)key * a.mat_stride + s;
    const double* __restrict__ L = a.ltab + (int64_t)key * a.ldl;
    double* __restrict__ Dr = a.dmats + ((int64_t)blockIdx.z * 3 + 2) * a.mat_stride + s;
    const double l1b = log1p(-a.slots[key].beta);
    double acc[kGgChunk];
#pragma unroll
    for (int i = 0; i < kGgChunk; ++i) acc[i] = 0.0;
    for (int j = 0; j < cc0; ++j) {                    // every c of the chunk lies above j
        const double p = Pt[(int64_t)j * a.ldp];
#pragma unroll
        for (int i = 0; i < kGgChunk; ++i) acc[i] = fma(L[cc0 - j + i], p, acc[i]);
    }
#pragma unroll
    for (int jj = 0; jj < kGgChunk; ++jj) {
        const int c = cc0 + jj;
        if (c > a.M) break;
        const double p = Pt[(int64_t)c * a.ldp];
        Dr[(int64_t)c * a.ldp] = fma(l1b, p, acc[jj]);
#pragma unroll
        for (int i = jj + 1; i < kGgChunk; ++i) acc[i] = fma(L[i - jj], p, acc[i]);
    }
}

// grid (cols / 64, leaves of the depth): lanes along f, the four waves a quarter of the parent's sizes each (gain_posterior_dense_leaf).
// sum_taps err[x][t] sum_s w[s] dP[s][c_t] for the three matrices; a missing cell's factor is exactly 1: its branch adds exactly 0.
__global__ __launch_bounds__(256) void gain_gradient_leaf_kernel(const GainGradArgs a) {
    __shared__ double red[4][64];
    const GainNodeOp op = a.ops[blockIdx.y];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 64 + x, ld = a.ld;
    const int64_t col = a.col[f];
    const int cnt = col >= 0 ? a.counts[(int64_t)op.taxon * a.counts_ld + col] : 0;
    const bool missing = count_is_missing(cnt), in = !missing && cnt <= a.M;
    const double* __restrict__ W = a.panels + op.W + f;
    const double* __restrict__ D = a.dmats + (int64_t)a.dmat_of[op.Pt / a.mat_stride] * 3 * a.mat_stride;
    const int chunk = (op.rows + 3) / 4, s_lo = y * chunk, s_hi = min(op.rows, s_lo + chunk);
    const int n_taps = a.err ? a.n_dev : 1, lo = a.err ? cnt - (a.n_dev - 1) / 2 : cnt;
    double g[3] = {0.0, 0.0, 0.0};
    for (int t = 0; t < n_taps; ++t) {                 // taps ascending; those outside [0, M] are dropped
        const int c = lo + t;
        const bool ok = in && c >= 0 && c <= a.M;
        double part[3] = {0.0, 0.0, 0.0};
        if (ok) {
            const double* __restrict__ dc = D + (int64_t)c * a.ldp;
            for (int s = s_lo; s < s_hi; ++s) {
                const double w = W[(int64_t)s * ld];
#pragma unroll
                for (int p = 0; p < 3; ++p) part[p] = fma(w, dc[(int64_t)p * a.mat_stride + s], part[p]);
            }
        }
        const double wt = ok && a.err ? a.err[(int64_t)cnt * a.n_dev + t] : 1.0;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const double dot = gain_dense_fold4(red, x, y, part[p]);
            if (ok) g[p] = fma(wt, dot, g[p]);
        }
    }
    if (y != 0) return;
    const double Z = exp(a.lnl[f]);
    const int64_t o = (int64_t)op.node * ld + f, plane = (int64_t)a.nn * ld;
#pragma unroll
    for (int p = 0; p < 3; ++p) a.res[o + p * plane] = missing ? 0.0 : g[p] / Z;
}
