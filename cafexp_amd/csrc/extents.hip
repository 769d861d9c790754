// Zero extents of the likelihood panels (interval propagation up the tree, once per scorer call, right after K1).
//
// A likelihood column is exactly zero far from the observed sizes: a leaf with count x contributes P_leaf[s][x], which
// underflows to 0 once s is many standard deviations from x; an interior child contributes sum_c P[s][c] L[c], zero
// wherever row s of the matrix has no non-zero entry inside the support of L; a node's vector is the product of its
// children's factors, zero wherever one of them is.  K1 publishes the non-zero extents of the matrices (per column of a
// leaf branch's matrix, per block of 16 rows of an interior branch's); this kernel turns them, per node, category and
// panel column, into an interval [lo, hi] of panel rows outside which the column is EXACTLY zero -- conservative (it may
// contain zeros, it never excludes a non-zero) -- and reduces the intervals of a 128-column tile to their hull.  K2 then
// runs, for a (row tile, column tile) pair, only the K tiles inside the intersection of the matrix extent and the panel
// extent: every product it leaves out has an exact zero in it, so no bit of any result changes (the reference has no
// counterpart: it multiplies all (M+1)^2 entries for every family, matrix_cache.cpp:28-57).
#include <algorithm>

#include "cafe_kernels.h"

namespace cafe {

// the interval of one panel column (node_level_kernel below runs it per column and reduces a tile's hull).  kext: the extents
// of the interior children's matrices, staged in LDS by the caller -- every column walks all their blocks, and from global
// memory each step of that walk is a dependent load.  mono[j]: first and last child size of child j's matrix do not decrease
// from block to block (a band: the caller checks it) -- the blocks that meet a child interval are then the run between
// the first block whose last size reaches the interval and the last block whose first size does, found by two binary
// searches instead of the walk; the same blocks, so the same interval.  Any other matrix takes the walk.
constexpr int kMaxExtBlocks = 128;                         // blocks of 16 parent sizes of the largest matrix order (2048)
__device__ inline int2 column_interval(const ExtArgs& a, const ExtNode& nd, int k, int col, const int32_t (*kext)[2 * kMaxExtBlocks],
                                       const int* mono) {
    int lo = 0, hi = a.M;
    const int half = a.n_dev > 0 ? (a.n_dev - 1) / 2 : 0;
    for (int l = 0; l < nd.n_leaf; ++l) {
        const int x = nd.cnt[(int64_t)nd.leaf_row[l] * nd.cnt_ld + col];
        const int32_t* e = a.leaf_ext + (int64_t)(k * a.n_pairs_leaf + nd.leaf_pair[l]) * a.leaf_ext_blocks * 2;
        int flo = 0x7fffffff, fhi = -1;
        if (a.n_dev <= 0) {
            flo = e[2 * x]; fhi = e[2 * x + 1];
        } else {
            for (int i = 0; i < a.n_dev; ++i) {             // sum_i err[x][i] P[s][x - half + i]: the hull of the taps that count
                const int c = x - half + i;
                if (c < 0 || c > a.M || a.err[(int64_t)x * a.n_dev + i] == 0.0) continue;
                flo = min(flo, e[2 * c]); fhi = max(fhi, e[2 * c + 1]);
            }
        }
        lo = max(lo, flo); hi = min(hi, fhi);
    }
    for (int j = 0; j < nd.n_inner; ++j) {
        const int cc = nd.inner_map[j] ? nd.inner_map[j][col] : col;
        const int32_t* ce = nd.inner_colext[j] + ((int64_t)k * nd.inner_cols[j] + cc) * 2;
        const int clo = ce[0], chi = ce[1];
        int flo = 0x7fffffff, fhi = -1;
        if (chi >= clo) {
            // parent sizes s = 16 b + 1 .. 16 b + 16 (panel rows s) of block b have non-zero matrix entries for the child
            // sizes [e[2b], e[2b+1]]; size 0 only reaches child size 0 (P[0][c] = delta(c, 0))
            const int32_t* e = kext[j];
            if (mono[j]) {
                int b1 = 0, n1 = a.kext_blocks;            // first block with e[2b+1] >= clo (kext_blocks: none)
                while (n1 > 0) { const int h = n1 >> 1; if (e[2 * (b1 + h) + 1] < clo) { b1 += h + 1; n1 -= h + 1; } else n1 = h; }
                int b2 = 0, n2 = a.kext_blocks;            // first block with e[2b] > chi; the one before it is the last that starts inside
                while (n2 > 0) { const int h = n2 >> 1; if (e[2 * (b2 + h)] <= chi) { b2 += h + 1; n2 -= h + 1; } else n2 = h; }
                if (b1 < b2) { flo = 16 * b1 + 1; fhi = 16 * (b2 - 1) + 16; }
            } else {
                for (int b = 0; b < a.kext_blocks; ++b)
                    if (e[2 * b + 1] >= clo && e[2 * b] <= chi) { flo = min(flo, 16 * b + 1); fhi = max(fhi, 16 * b + 16); }
            }
            if (clo == 0) { flo = 0; fhi = max(fhi, 0); }
            fhi = min(fhi, a.M);
        }
        lo = max(lo, flo); hi = min(hi, fhi);
    }
    if (hi < lo) { lo = 0x7fffffff; hi = -1; }
    return make_int2(lo, hi);
}

// ---- Magnitudes: K steps whose products underflow below the smallest denormal.
// The extents above leave out a product only when one factor is exactly zero.  A product of two non-zero factors below
// 2^-1075 has no effect either: all operands are non-negative, an accumulator that is 0 stays 0 and one that is not is at
// least 2^-1074 and does not move under round-to-nearest, whether the MFMA fuses its four products, chains them or rounds
// each one.  Three steps, all per call: (1) tables of the largest entries of this call's matrices, one pass over the pools;
// (2) upper bounds of the panels, propagated with the intervals, level by level; (3) per (op, category, column tile,
// 16-row block) the k-steps that can still matter, cut out of the exact interval.

// upper bound of log2(v) in 1/256, v >= 0
__device__ inline int32_t mag_of(double v) {
    if (!(v > 0.0)) return kMagNone;
    int e;
    const double m = frexp(v, &e);                         // v = m 2^e, m in [0.5, 1)
    return e * kMagUnit + (int32_t)ceilf(log2f((float)m) * (float)kMagUnit) + 1;
}

// Both tables in one launch, the block index decides the role (block-uniform):
//   leaf role     one workgroup per (32 row steps, 64 counts x, row-major slot): rows s = 4 r .. 4 r + 3 over the counts x <= M.
//                 The table is [slot][x][r] -- its reader walks r -- while the matrix is read along x: the workgroup turns its
//                 64 x 32 tile through LDS and stores 32 consecutive r per count (128-byte runs; one r per workgroup meant a
//                 4-byte store per line);
//   k-major role  one workgroup per (k-step, k-major slot): the four matrix rows c = 4 ks .. 4 ks + 3 over all parent sizes.
// The leaf workgroups come first in the grid; the k-major ones follow and stream the larger pool behind them.
constexpr int kLeafR = 32, kLeafX = 64, kLeafLd = kLeafR + 1;
__global__ __launch_bounds__(256) void mag_tables_kernel(const MagArgs a, int leaf_blocks, int leaf_rb, int leaf_xb) {
    extern __shared__ double s_dyn[];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < leaf_blocks) {
        int32_t* s_t = reinterpret_cast<int32_t*>(s_dyn);  // [kLeafX][kLeafLd]
        int id = blockIdx.x;
        const int rb = id % leaf_rb; id /= leaf_rb;
        const int xb = id % leaf_xb, slot = id / leaf_xb;
        const double* P = a.lpool.base + (int64_t)slot * a.lpool.stride;
        const int xl = tid & (kLeafX - 1), x = xb * kLeafX + xl, w = tid / kLeafX;
        const bool x_in = x <= a.M && x < a.lpool.n;
        // all 32 loads of a lane first (rows past the matrix and counts past M: the entry at (0, 0) in their place, not used)
        double v[kLeafR / 4][4];
#pragma unroll
        for (int i = 0; i < kLeafR / 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int s = 4 * (rb * kLeafR + w + 4 * i) + q;
                v[i][q] = P[x_in && s < a.lpool.n ? (int64_t)s * a.lpool.ld + x : 0];
            }
#pragma unroll
        for (int i = 0; i < kLeafR / 4; ++i) {
            const int rl = w + 4 * i, r = rb * kLeafR + rl;
            double mx = (r == 0 && x == 0) ? 1.0 : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (x_in && 4 * r + q < a.lpool.n) mx = fmax(mx, v[i][q]);
            s_t[xl * kLeafLd + rl] = mag_of(mx);
        }
        __syncthreads();
        for (int i = tid; i < kLeafX * kLeafR; i += 256) {
            const int ox = i / kLeafR, rl = i % kLeafR, xx = xb * kLeafX + ox, r = rb * kLeafR + rl;
            if (xx <= a.M && xx < a.lpool.n && r < a.n_rsteps) a.lt[((int64_t)slot * (a.M + 1) + xx) * a.n_rsteps + r] = s_t[ox * kLeafLd + rl];
        }
        return;
    }
    const int kid = blockIdx.x - leaf_blocks, ks = kid % a.n_ksteps, slot = kid / a.n_ksteps;
    const int ncol = min(a.kpool.n - 1, 2048);             // parent sizes 1 .. n - 1 are columns 0 .. n - 2
    double* s_max = s_dyn;
    double* s_sum = s_dyn + ncol;
    const double* P = a.kpool.base + (int64_t)slot * a.kpool.stride + (int64_t)ks * 4 * a.kpool.ld;
    for (int j = tid; j < ncol; j += 256) {
        double mx = 0.0, sm = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = ks * 4 + c < a.kpool.k_valid ? P[(int64_t)c * a.kpool.ld + j] : 0.0;
            mx = fmax(mx, v); sm += v;
        }
        s_max[j] = mx; s_sum[j] = sm;
    }
    __syncthreads();
    const int nb = a.kpool.ext_blocks;
    for (int b = tid; b < nb; b += 256) {
        double mx = 0.0;
        for (int j = 16 * b; j < 16 * b + 16 && j < ncol; ++j) mx = fmax(mx, s_max[j]);
        a.a16[((int64_t)slot * a.n_ksteps + ks) * nb + b] = mag_of(mx);
    }
    for (int r = tid; r < a.n_rsteps; r += 256) {
        double mx = (r == 0 && ks == 0) ? 1.0 : 0.0;       // parent size 0: P[0][c] = delta(c, 0)
        for (int s = max(4 * r, 1); s < 4 * r + 4 && s - 1 < ncol; ++s) mx = fmax(mx, s_sum[s - 1]);
        a.t4[((int64_t)slot * a.n_ksteps + ks) * a.n_rsteps + r] = mag_of(mx);
    }
}

hipError_t launch_magnitude_tables(const MagArgs& a, hipStream_t stream) {
    const int leaf_rb = (a.n_rsteps + kLeafR - 1) / kLeafR, leaf_xb = (a.M + 1 + kLeafX - 1) / kLeafX;
    const int leaf_blocks = a.n_lslots > 0 ? leaf_rb * leaf_xb * a.n_lslots : 0;
    const int k_blocks = a.n_kslots > 0 ? a.n_ksteps * a.n_kslots : 0;
    if (leaf_blocks + k_blocks <= 0) return hipSuccess;
    const int ncol = std::min(a.kpool.n - 1, 2048);
    const size_t lds = std::max(sizeof(double) * 2 * (size_t)std::max(ncol, 0), sizeof(int32_t) * kLeafX * kLeafLd);
    (void)hipGetLastError();
    hipLaunchKernelGGL(mag_tables_kernel, dim3(leaf_blocks + k_blocks), dim3(256), lds, stream, a, leaf_blocks, leaf_rb, leaf_xb);
    return hipGetLastError();
}

// Upper bounds of a node's panel per (category, 128-column tile, step of 4 rows), after the node's extents (it reads the
// tile's hull) and its children's bounds.  They must dominate the COMPUTED values, not the exact ones:
//   leaf factor      max of the leaf's table over the counts that occur in the tile;
//   interior factor  log2 sum_ks 2^(t4[ks][r] + child bound[ks]), the child bound taken over the child tiles that the tile's
//                    columns map to: sum_c P[s][c] L[c][f] <= sum_ks (sum_{c in ks} P[s][c]) max_{c in ks} L[c][f];
//   node             the sum over its factors + kMagSlack, never below kMagFloor inside the exact extent: what the roundings
//                    of the sums and products add is a factor (1 + 2^-53)^n and, in the denormal range, at most 2^-1075 per
//                    operation -- under 2^-1063 in all, which a bound of at least 2^-1050 swallows within the slack.
// The interior factor's sum runs in float, spread over kLevelPhases waves (wave w: the k-steps ks = w mod kLevelPhases of a
// row's range, ascending in batches of kBoundBatch, as a running maximum `top` and S = sum 2^((v - top) / 256), rescaled
// once per batch) and combined in the fixed order w = 0, 1, ...: deterministic, no float atomics.  Every term is at most 1,
// so against the exact sum S carries a relative error of at most (terms + rescales + combines) x (2^-24 of the addition or
// multiplication + 2^-22 of the exponential) -- with up to 512 k-steps, counting a term and a rescale for each, under
// 1030 x 1.25 x 2^-22 < 2^-11.6.  The sum is therefore scaled by (1 + 2^-11) before its logarithm is taken (in float: the factor
// leaves 1.8e-4 of the sum, 0.067 of a unit, over; log2f of a sum of at most 512 is off by under 2e-6 and the product with
// 256 by under 2e-4 of a unit) and rounded up to the unit: the factor's bound dominates the exact log2 sum
// with no further unit added (the factor costs 0.18 of a unit; a unit per partial sum would cost one each, and the serial
// float sum this replaces added one after its ceiling: the bounds come out a unit tighter per interior factor, not looser).
// The loops over counts, child tiles and k-steps read tables far larger than the caches: each batches independent loads in
// front of the arithmetic (kListBatch per list, kBoundBatch per wave and round of k-steps; one after the other they cost a
// memory round trip per item: 7.3 ms per bench call).  A round is kLevelPhases x kBoundBatch = 16 k-steps: the rows' ranges
// at the bench order are short, and every k-step of a round is computed whether the range holds it or not (rounds of 64:
// 4.06 ms per bench call for the kernel, of 32: 3.5, of 16: 3.2).
//
// One launch per tree level: a workgroup owns up to kLevelTiles consecutive column tiles of one (node, category).  It first
// runs the intervals of its columns (column_interval) and reduces each tile's hull, which stays in LDS; without magnitude
// tables (ExtArgs::t4 null) it ends there.  Then the bounds, for the row steps inside the hulls only (outside they say
// kMagNone): every t4 entry a lane loads serves all the workgroup's tiles, which differ only in their child-tile maxima.
// A workgroup reads what earlier levels wrote and what it wrote itself, never another workgroup's output of its own level.
constexpr int kLevelThreads = 256, kLevelTiles = 4, kLevelPhases = kLevelThreads / 64, kBoundBatch = 4, kListBatch = 16;
static_assert(kLevelPhases == kLevelTiles && kLevelTiles == 4 && kLevelThreads == 2 * kBN,
              "the combine step maps wave -> tile, s_cb holds the tiles of a k-step as an int4, the intervals run two tiles per pass");
__global__ __launch_bounds__(kLevelThreads, 4) void node_level_kernel(const ExtArgs a, const int tiles_per_block) {
    const ExtNode& nd = a.nodes[a.first + blockIdx.z];
    const int nct = nd.cols / kBN, ct0 = blockIdx.x * tiles_per_block;
    if (ct0 >= nct) return;                                // (levels are launched as wide as their widest node; block-uniform)
    const int nt = min(tiles_per_block, nct - ct0);        // <= kLevelTiles
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nr = a.n_rsteps, nk = a.n_ksteps;
    __shared__ int32_t s_acc[kLevelTiles][kMaxSteps];
    __shared__ int4 s_cb[kMaxSteps];                        // the child's bound per k-step, the workgroup's four tiles side by side
    __shared__ int s_list[kLevelTiles][kBN];               // the distinct counts / child tiles of a tile's columns
    __shared__ unsigned s_bits[kLevelTiles][kMaxSteps / 8];    // counts 0 .. 2047
    __shared__ int s_n[kLevelTiles], s_klo[kLevelTiles], s_khi[kLevelTiles];
    __shared__ int s_wlo[2 * kLevelTiles], s_whi[2 * kLevelTiles], s_lo[kLevelTiles], s_hi[kLevelTiles], s_rlo[kLevelTiles], s_rhi[kLevelTiles];
    __shared__ int32_t s_ptop[kLevelPhases][kLevelTiles][64];
    __shared__ float s_psum[kLevelPhases][kLevelTiles][64];
    __shared__ int32_t s_kext[kMaxExtChildren][2 * kMaxExtBlocks];     // the interior children's matrix extents (this category)
    __shared__ int s_mono[kMaxExtChildren];                // the child's matrix extents do not decrease from block to block
    if (tid < kMaxExtChildren) s_mono[tid] = 1;
    __syncthreads();
    for (int j = 0; j < nd.n_inner; ++j)
        for (int i = tid; i < 2 * a.kext_blocks; i += kLevelThreads) {
            const int32_t* g = a.kext + (int64_t)(k * a.n_pairs_inner + nd.inner_pair[j]) * a.kext_blocks * 2;
            s_kext[j][i] = g[i];
            if (i >= 2 && g[i] < g[i - 2]) s_mono[j] = 0;   // (first sizes are the even entries, last sizes the odd ones)
        }
    __syncthreads();

    // ---- intervals: 128 threads per tile, two tiles at a time (a wave lies inside one tile)
    // (both passes' intervals before either's stores: the chains of dependent loads of the two then run side by side)
    int2 iv[kLevelTiles * kBN / kLevelThreads];
#pragma unroll
    for (int p = 0; p < kLevelTiles * kBN / kLevelThreads; ++p)
        if (tid + p * kLevelThreads < nt * kBN) iv[p] = column_interval(a, nd, k, ct0 * kBN + tid + p * kLevelThreads, s_kext, s_mono);
#pragma unroll
    for (int p = 0; p < kLevelTiles * kBN / kLevelThreads; ++p) {
        const int i = tid + p * kLevelThreads;
        if (i >= nt * kBN) continue;                       // (whole waves: a wave lies inside one tile)
        int lo = iv[p].x, hi = iv[p].y;
        int32_t* out = nd.colext + ((int64_t)k * nd.cols + ct0 * kBN + i) * 2;
        out[0] = lo; out[1] = hi;
        for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_down(lo, off)); hi = max(hi, __shfl_down(hi, off)); }
        if (lane == 0) { s_wlo[i >> 6] = lo; s_whi[i >> 6] = hi; }
    }
    __syncthreads();
    if (tid < nt) {                                        // hull over the 128 columns of a tile
        const int lo = min(s_wlo[2 * tid], s_wlo[2 * tid + 1]), hi = max(s_whi[2 * tid], s_whi[2 * tid + 1]);
        int32_t* t = nd.tileext + ((int64_t)k * nct + ct0 + tid) * 2;
        t[0] = lo; t[1] = hi;
        s_lo[tid] = lo; s_hi[tid] = hi;
        s_rlo[tid] = hi >= lo ? lo / 4 : nr; s_rhi[tid] = hi >= lo ? min(hi / 4, nr - 1) : -1;
    }
    if (!a.t4) return;                                     // (a kernel argument: uniform)
    __syncthreads();
    // the row steps inside a hull: all of a tile's, and of the workgroup's tiles together
    int rlo = nr, rhi = -1;
    for (int c = 0; c < nt; ++c) { rlo = min(rlo, s_rlo[c]); rhi = max(rhi, s_rhi[c]); }
    for (int i = tid; i < kLevelTiles * kMaxSteps; i += kLevelThreads) (&s_acc[0][0])[i] = 0;

    // ---- leaf factors: the largest table entry over the distinct counts of the tile's columns
    for (int l = 0; l < nd.n_leaf; ++l) {
        __syncthreads();
        for (int i = tid; i < kLevelTiles * (kMaxSteps / 8); i += kLevelThreads) (&s_bits[0][0])[i] = 0;
        if (tid < kLevelTiles) s_n[tid] = 0;
        __syncthreads();
        for (int i = tid; i < nt * kBN; i += kLevelThreads) {
            const int c = i / kBN;
            const int x = nd.cnt[(int64_t)nd.leaf_row[l] * nd.cnt_ld + ct0 * kBN + i];
            if (!(atomicOr(&s_bits[c][x >> 5], 1u << (x & 31)) & (1u << (x & 31)))) s_list[c][atomicAdd(&s_n[c], 1)] = x;    // the first to set it
        }
        __syncthreads();
        const int32_t* lt = a.lt + (int64_t)(k * a.n_pairs_leaf + nd.leaf_pair[l]) * (a.M + 1) * nr;
        const int span = rhi - rlo + 1;
        for (int i = tid; i < nt * span; i += kLevelThreads) {
            const int c = i / span, r = rlo + i % span;
            if (r < s_rlo[c] || r > s_rhi[c]) continue;
            const int n = s_n[c];
            int32_t m = kMagNone;
            for (int i0 = 0; i0 < n; i0 += kListBatch) {
                int32_t v[kListBatch];
#pragma unroll
                for (int q = 0; q < kListBatch; ++q) v[q] = lt[(int64_t)s_list[c][min(i0 + q, n - 1)] * nr + r];
#pragma unroll
                for (int q = 0; q < kListBatch; ++q) m = max(m, v[q]);
            }
            s_acc[c][r] = (m == kMagNone || s_acc[c][r] == kMagNone) ? kMagNone : s_acc[c][r] + m;
        }
    }

    // ---- interior factors
    for (int j = 0; j < nd.n_inner; ++j) {
        __syncthreads();
        for (int i = tid; i < kLevelTiles * (kMaxSteps / 8); i += kLevelThreads) (&s_bits[0][0])[i] = 0;
        if (tid < kLevelTiles) { s_n[tid] = 0; s_klo[tid] = nk; s_khi[tid] = -1; }
        __syncthreads();
        for (int i = tid; i < nt * kBN; i += kLevelThreads) {
            const int c = i / kBN, col = ct0 * kBN + i;
            const int t = (nd.inner_map[j] ? nd.inner_map[j][col] : col) / kBN;
            // (tiles past the bitmap enter the list once per column: that costs loads and changes no maximum)
            if (t >= kMaxSteps * 4 || !(atomicOr(&s_bits[c][t >> 5], 1u << (t & 31)) & (1u << (t & 31)))) s_list[c][atomicAdd(&s_n[c], 1)] = t;
        }
        __syncthreads();
        // the child's bound per k-step: the maximum over the child tiles the tile's columns map to -- for the k-steps that the
        // matrix blocks of the hulls' rows reach (the union of the rows' ranges below); the others are not looked at
        const int slot = k * a.n_pairs_inner + nd.inner_pair[j];
        const int32_t* e = s_kext[j];
        int kmin = nk, kmax = -1;
        if (rhi >= rlo) {
            for (int b = max(4 * rlo - 1, 0) / 16; b <= (4 * rhi + 2) / 16 && b < a.kext_blocks; ++b)
                if (e[2 * b + 1] >= e[2 * b]) { kmin = min(kmin, e[2 * b] / 4); kmax = max(kmax, e[2 * b + 1] / 4); }
            if (rlo == 0) kmin = 0, kmax = max(kmax, 0);
            kmax = min(kmax, nk - 1);
        }
        const int kspan = max(kmax - kmin + 1, 0);
        for (int i = tid; i < nt * nk; i += kLevelThreads)
            if (i % nk < kmin || i % nk > kmax) (&s_cb[i % nk].x)[i / nk] = kMagNone;
        const int32_t* cb = nd.inner_bound[j] + (int64_t)k * (nd.inner_cols[j] / kBN) * nr;
        for (int i = tid; i < nt * kspan; i += kLevelThreads) {
            const int c = i / kspan, ks = kmin + i % kspan, n = s_n[c];
            int32_t m = kMagNone;
            for (int i0 = 0; i0 < n; i0 += kListBatch) {
                int32_t v[kListBatch];
#pragma unroll
                for (int q = 0; q < kListBatch; ++q) v[q] = cb[(int64_t)s_list[c][min(i0 + q, n - 1)] * nr + ks];
#pragma unroll
                for (int q = 0; q < kListBatch; ++q) m = max(m, v[q]);
            }
            (&s_cb[ks].x)[c] = m;
            if (m != kMagNone) { atomicMin(&s_klo[c], ks); atomicMax(&s_khi[c], ks); }
        }
        __syncthreads();
        int cklo = nk, ckhi = -1;                          // the k-steps where some tile's child bound says anything
#pragma unroll
        for (int c = 0; c < kLevelTiles; ++c)
            if (c < nt) { cklo = min(cklo, s_klo[c]); ckhi = max(ckhi, s_khi[c]); }
        const int32_t* t4 = a.t4 + (int64_t)slot * nk * nr;
        // 64 row steps at a time, lane = row step; wave w sums the k-steps = w mod kLevelPhases of the row's range
        for (int r0 = rlo; r0 <= rhi; r0 += 64) {
            const int r = r0 + lane;
            int32_t top[kLevelTiles];
            float sum[kLevelTiles];                        // (a sum means nothing while its top says "none": see the rounds below)
#pragma unroll
            for (int c = 0; c < kLevelTiles; ++c) { top[c] = kMagNone; sum[c] = 0.f; }
            if (r <= rhi) {
                // the k-steps inside the child's support and inside the non-zero extents of the matrix blocks that hold the parent
                // sizes 4 r .. 4 r + 3 (block b: sizes 16 b + 1 .. 16 b + 16; size 0 only reaches child size 0)
                int klo = nk, khi = -1;
                for (int b = max(4 * r - 1, 0) / 16; b <= (4 * r + 2) / 16 && b < a.kext_blocks; ++b)
                    if (e[2 * b + 1] >= e[2 * b]) { klo = min(klo, e[2 * b] / 4); khi = max(khi, e[2 * b + 1] / 4); }
                if (r == 0) klo = 0, khi = max(khi, 0);
                klo = max(klo, cklo); khi = min(min(khi, ckhi), nk - 1);
                // (rounds of kLevelPhases x kBoundBatch k-steps on an absolute grid, not from klo: klo and khi depend on which
                // tiles share the workgroup, and so would the batches and the roundings of a tile's sum; on the grid a tile's
                // sum meets the same terms in the same batches whatever its neighbours are -- the steps a wider range adds say
                // "none" for it and add exact zeros -- so its bound has the same bits for any number of tiles per workgroup)
                for (int k0 = klo / (kLevelPhases * kBoundBatch) * (kLevelPhases * kBoundBatch) + wave; k0 <= khi; k0 += kLevelPhases * kBoundBatch) {
                    int32_t tv[kBoundBatch];
#pragma unroll
                    for (int q = 0; q < kBoundBatch; ++q) tv[q] = t4[(int64_t)min(max(k0 + kLevelPhases * q, klo), khi) * nr + r];
                    // a batch at a time: the new maxima first, then one rescale of each sum and one term per k-step and tile, no
                    // branch per term (a term that says "none" is 2^(-2^20) = 0 against any maximum; v_exp_f32 itself: a term
                    // below 2^-126 of the largest counts as 0, 512 of them are far inside the factor above)
                    // (while a tile has met no term at all its maximum says "none" too and the sum collects ones: the first real
                    // maximum rescales them by 2^(-2^20) = 0, and the combine step leaves out a partial sum whose maximum is "none")
                    int32_t m[kLevelTiles];
#pragma unroll
                    for (int c = 0; c < kLevelTiles; ++c) m[c] = top[c];
#pragma unroll
                    for (int q = 0; q < kBoundBatch; ++q) {
                        const int ks = k0 + kLevelPhases * q;
                        const int4 cv4 = s_cb[min(max(ks, klo), khi)];
                        const int32_t cv[kLevelTiles] = {cv4.x, cv4.y, cv4.z, cv4.w};
                        if (ks < klo || ks > khi) tv[q] = kMagNone;
#pragma unroll
                        for (int c = 0; c < kLevelTiles; ++c)
                            if (c < nt && tv[q] != kMagNone && cv[c] != kMagNone) m[c] = max(m[c], tv[q] + cv[c]);
                    }
#pragma unroll
                    for (int c = 0; c < kLevelTiles; ++c) {
                        sum[c] *= __builtin_amdgcn_exp2f((float)(top[c] - m[c]) * (1.f / kMagUnit));
                        top[c] = m[c];
                    }
#pragma unroll
                    for (int q = 0; q < kBoundBatch; ++q) {
                        const int4 cv4 = s_cb[min(max(k0 + kLevelPhases * q, klo), khi)];
                        const int32_t cv[kLevelTiles] = {cv4.x, cv4.y, cv4.z, cv4.w};
#pragma unroll
                        for (int c = 0; c < kLevelTiles; ++c) {
                            if (c >= nt) continue;
                            const int32_t v = (tv[q] != kMagNone && cv[c] != kMagNone) ? tv[q] + cv[c] : kMagNone;
                            sum[c] += __builtin_amdgcn_exp2f((float)(v - m[c]) * (1.f / kMagUnit));
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kLevelTiles; ++c) { s_ptop[wave][c][lane] = top[c]; s_psum[wave][c][lane] = sum[c]; }
            __syncthreads();
            {   // thread -> (tile, row step of the chunk): the partial sums in the order of the waves
                const int c = wave, rr = r0 + lane;
                if (c < nt && rr >= s_rlo[c] && rr <= s_rhi[c]) {
                    int32_t T = kMagNone;
#pragma unroll
                    for (int w = 0; w < kLevelPhases; ++w) T = max(T, s_ptop[w][c][lane]);
                    int32_t f = kMagNone;
                    if (T != kMagNone) {
                        float S = 0.f;
#pragma unroll
                        for (int w = 0; w < kLevelPhases; ++w)
                            if (s_ptop[w][c][lane] != kMagNone) S += s_psum[w][c][lane] * exp2f((float)(s_ptop[w][c][lane] - T) * (1.f / kMagUnit));
                        f = T + (int32_t)ceilf(log2f(S * (1.f + 0x1p-11f)) * (float)kMagUnit);
                    }
                    s_acc[c][rr] = (f == kMagNone || s_acc[c][rr] == kMagNone) ? kMagNone : s_acc[c][rr] + f;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = tid; i < nt * nr; i += kLevelThreads) {
        const int c = i / nr, r = i % nr, lo = s_lo[c], hi = s_hi[c];
        nd.bound[((int64_t)k * nct + ct0 + c) * nr + r] =
            (hi >= lo && 4 * r + 3 >= lo && 4 * r <= hi) ? max(s_acc[c][r], kMagFloor) + kMagSlack : kMagNone;
    }
}

// Tiles a workgroup owns (ExtArgs::level_tiles, or 0: chosen here): four where that still leaves the level's grid ten
// workgroups per CU's worth of tiles, two from five (five are resident per CU; with fewer tiles one workgroup each keeps
// more CUs busy).  A tile's bound does not depend on the choice (node_level_kernel: the grid of its rounds is absolute).
hipError_t launch_node_level(const ExtArgs& a, int max_col_tiles, int n_categories, hipStream_t stream) {
    if (a.count <= 0) return hipSuccess;
    const int64_t tiles = (int64_t)max_col_tiles * n_categories * a.count, cus = std::max(1, a.n_cu);
    int per_block = !a.t4 ? 2 : tiles >= 10 * cus ? kLevelTiles : tiles >= 5 * cus ? 2 : 1;
    if (a.level_tiles == 1 || a.level_tiles == 2 || a.level_tiles == kLevelTiles) per_block = a.level_tiles;
    (void)hipGetLastError();
    hipLaunchKernelGGL(node_level_kernel, dim3((max_col_tiles + per_block - 1) / per_block, n_categories, a.count), dim3(kLevelThreads), 0,
                       stream, a, per_block);
    return hipGetLastError();
}

// Joint K ranges (GemmOp::jr): lane = 16-row block of the op's matrix.  The exact interval is the block's matrix extent cut
// by the panel's (an empty panel extent: row 0, so that the panel receives its zeros); with magnitude tables the interval
// shrinks from both ends while (largest entry of the block in the k-step) x (bound of the panel's rows of the k-step) lies
// below 2^-1100.  The ranges only ever shrink: no MFMA reads a panel row the assemble pass left unwritten.
// One wave per (op, category, column tile), four column tiles per workgroup: the lanes of a wave are the matrix's blocks
// (ext_blocks + kRangePad <= 136: up to three per lane), and a lane looks from both ends of its interval at once,
// kRangeBatch k-steps from either end per look (independent loads).  The first and the last k-step that count do not depend
// on how many are looked at together.
constexpr int kRangeWaves = 4, kRangeBatch = 8;
__global__ __launch_bounds__(64 * kRangeWaves) void range_kernel(const RangeArgs a) {
    const GemmOp& o = a.ops[blockIdx.z];
    if (!o.jr || (int)blockIdx.x * kRangeWaves >= o.jr_nct) return;     // (block-uniform)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ct = blockIdx.x * kRangeWaves + wave, cat = blockIdx.y, nb = a.ext_blocks;
    const bool live = ct < o.jr_nct, mag = a.a16 && o.bbound;
    __shared__ int32_t s_ball[kRangeWaves][kMaxSteps];      // the panel's bound per k-step
    const int32_t* s_b = s_ball[wave];
    if (mag) {
        if (live) {
            const int32_t* B = o.bbound + ((int64_t)cat * o.jr_nct + ct) * a.n_rsteps;
            for (int i = lane; i < a.n_ksteps; i += 64) s_ball[wave][i] = B[i];
        }
        __syncthreads();
    }
    if (!live) return;
    const int slot = o.slot[cat];
    int plo = 0, phi = a.k_valid - 1;
    if (o.bext) {
        const int32_t* be = o.bext + ((int64_t)cat * o.jr_nct + ct) * 2;
        plo = be[0]; phi = min(be[1], phi);
        if (be[1] < be[0]) { plo = 0; phi = 0; }
    }
    for (int b = lane; b < nb + kRangePad; b += 64) {
        int slo = 1, shi = 0;
        if (b < nb) {
            const int32_t* e = a.aext + ((int64_t)slot * nb + b) * 2;
            const int lo = max(e[0], plo), hi = min(e[1], phi);
            if (hi >= lo) {
                slo = lo / 4; shi = hi / 4;
                if (mag) {
                    // a step counts when it may reach 2^-1100
                    const int32_t* A = a.a16 + (int64_t)slot * a.n_ksteps * nb + b;
                    const int first = slo, last = shi;
                    bool ffound = false, lfound = false;
                    while ((!ffound && slo <= last) || (!lfound && shi >= first)) {
                        int32_t vf[kRangeBatch], vl[kRangeBatch];
#pragma unroll
                        for (int i = 0; i < kRangeBatch; ++i) {
                            vf[i] = A[(int64_t)min(slo + i, last) * nb];
                            vl[i] = A[(int64_t)max(shi - i, first) * nb];
                        }
#pragma unroll
                        for (int i = 0; i < kRangeBatch; ++i) {
                            if (!ffound) { if (slo <= last && vf[i] + s_b[slo] >= kSkipBelow) ffound = true; else if (slo <= last) ++slo; }
                            if (!lfound) { if (shi >= first && vl[i] + s_b[shi] >= kSkipBelow) lfound = true; else if (shi >= first) --shi; }
                        }
                    }
                    if (!ffound || !lfound || slo > shi) { slo = 1; shi = 0; }
                }
            }
        }
        const_cast<int32_t*>(o.jr)[((int64_t)cat * o.jr_nct + ct) * (nb + kRangePad) + b] = slo | (shi << 16);
    }
}

hipError_t launch_joint_ranges(const RangeArgs& a, int max_col_tiles, int n_categories, hipStream_t stream) {
    if (a.n_ops <= 0 || !a.aext) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(range_kernel, dim3((max_col_tiles + kRangeWaves - 1) / kRangeWaves, n_categories, a.n_ops), dim3(64 * kRangeWaves), 0,
                       stream, a);
    return hipGetLastError();
}

constexpr int kPlanTail = 2;
// Tile lists of the K2 launches of a call (PlanLaunch, cafe_kernels.h): one wave per (XCD, launch), lane = workgroup.
// Cost of a tile = its K tiles + PlanLaunch::fixed.  With the full grid (64 workgroups per XCD) workgroups j and j + 32 share
// a CU, and the one dispatched first (j < 32) wins the MFMA arbitration: given equal lists it ALWAYS finishes first, 8 % of
// the launch earlier, and the CU runs one workgroup to the end (tools/gemm_timeline.py).  The planner therefore charges a
// tile `bias` percent less to j < 32 and as much more to j >= 32, so that the favoured workgroup takes more of the work.
// What a K tile costs workgroup w of an XCD, in percent of the mean: the workgroups of a CU do not share its matrix pipe
// evenly -- the one dispatched first wins the arbitration (with three per CU and equal lists they finish at 2 672 / 3 200 /
// 3 503 us of a 3 563 us launch: tools/k2_tile_costs.py) -- so the planner charges the favoured ones less and they take more
// of the work.  Full grids only (local indices j, j + 32, ... share a CU).
__device__ inline int plan_weight(const PlanLaunch& L, const int* bias3, int nlb, int w) {
    if (nlb == 64 && L.bias) return w < 32 ? 100 - L.bias : 100 + L.bias;
    // (bias3: PlanLaunch::bias3 staged in LDS -- indexing the member of the kernel's register copy of L would put the whole copy
    // into scratch memory)
    if (nlb == 96 || nlb == 128) return bias3[w >> 5];
    return 100;
}

// Tile t of XCD `xcd`'s list -- the concatenation of the lists of the launch's ops, each pair-major with the row tile
// fastest (the order prune_gemm.hip's decode assumes) -- as a plan entry: x = op << 24 | index in the op's own list,
// y = first K tile << 16 | K tiles.  s_first[o]: where op o's tiles start in the XCD's list (s_first[n_ops] = all).
__device__ inline int2 plan_tile_entry(const PlanLaunch& L, const int* s_first, int xcd, int t) {
    int op = 0;
    while (op + 1 < L.n_ops && t >= s_first[op + 1]) ++op;
    const GemmOp& o = L.ops[op];
    const int tl = t - s_first[op];
    const int nrt = o.n_row_tiles, nct = L.uniform_ld > 0 ? L.uniform_ld / kBN : o.n_col_tiles;
    const int row_tile = tl % nrt;
    const int pair = xcd + 8 * (tl / nrt);
    const int ct = pair % nct, cat = pair / nct;
    int lo = 0, hi = L.k_valid - 1, zlo = 0;
    if (L.aext) {
        // the hull of the row blocks' joint ranges (range_kernel; entries past the matrix's last block say "none")
        const int32_t* e = o.jr + ((int64_t)cat * o.jr_nct + (ct & o.jr_ct_mask)) * (L.ext_blocks + kRangePad) + row_tile * L.mi;
        int slo = 0x7fff, shi = -1;
        for (int b = 0; b < L.mi; ++b) {
            const int l = e[b] & 0xFFFF, h = e[b] >> 16;
            if (h >= l) { slo = min(slo, l); shi = max(shi, h); }
        }
        lo = slo * 4; hi = shi * 4 + 3;
        if (o.bext) {
            // (rows of B outside its tile extent may never have been written: the assemble pass leaves them out, leaf_reduce.hip)
            const int32_t* be = o.bext + ((int64_t)cat * nct + ct) * 2;
            if (be[1] >= be[0]) zlo = be[0];
        }
        if (shi < slo) { lo = zlo; hi = zlo; }             // an all-zero tile still runs one K tile: the panel must receive its zeros
        hi = min(hi, L.k_valid - 1);
    }
    return make_int2((op << 24) | tl, ((lo / L.kb) << 16) | (hi / L.kb - lo / L.kb + 1));
}

// The last kPlanTail rounds are dealt as ONE batch, longest tile first, each to the workgroup with the least load at that
// moment (a workgroup may then end up with a tile more or less than its neighbours: lists have kPlanSlack spare entries).
// The rounds before them are dealt in chunks of kPlanChunk rounds, one wave per chunk (blockIdx.z), each balancing its own
// rounds from a load of zero -- a launch of a whole tree level has hundreds of rounds, and one wave dealing them one after
// the other took 1.8 ms in front of the first K2 launch of a config-4 call.
constexpr int kPlanChunk = 8;
__global__ __launch_bounds__(kPlanLanes) void tile_plan_kernel(const PlanLaunch* __restrict__ launches) {
    // (a copy in registers: the lists written below might alias the descriptor for all the compiler knows, and every field
    // would be re-read from memory at each use -- the serial tail loop then paid a memory round trip per item)
    const PlanLaunch L = launches[blockIdx.y];
    const int xcd = blockIdx.x, lane = threadIdx.x;         // lane = workgroup of the XCD (< blocks_per_xcd <= kPlanLanes)
    const int nlb = L.blocks_per_xcd;
    __shared__ int s_first[kMaxGroupOps + 1], s_bias3[4];
    if (lane < 4) s_bias3[lane] = launches[blockIdx.y].bias3[lane];
    if (lane == 0) {
        int acc = 0;
        for (int o = 0; o < L.n_ops; ++o) {
            s_first[o] = acc;
            const int nct = L.uniform_ld > 0 ? L.uniform_ld / kBN : L.ops[o].n_col_tiles;
            acc += ((L.n_categories * nct - xcd + 7) >> 3) * L.ops[o].n_row_tiles;
        }
        s_first[L.n_ops] = acc;
    }
    __syncthreads();
    const int n_tiles = s_first[L.n_ops];
    // (two workgroups per CU, 64 per XCD: j and j + 32 share a CU and the first-dispatched one runs `bias` percent faster)
    __shared__ int s_load[kPlanLanes], s_cost[kPlanLanes], s_who[kPlanLanes];
    __shared__ int t_cost[kPlanTail * kPlanLanes], t_x[kPlanTail * kPlanLanes], t_y[kPlanTail * kPlanLanes], t_by_rank[kPlanTail * kPlanLanes];
    s_load[lane] = 0;
    __syncthreads();
    const int head = max(0, (n_tiles + nlb - 1) / nlb - kPlanTail);      // full rounds dealt one by one
    const int n_chunks = max(1, (head + kPlanChunk - 1) / kPlanChunk), chunk = blockIdx.z;
    if (chunk >= n_chunks) return;                          // (block-uniform: the grid is as deep as the launch with most rounds)
    // the chunk's entries first, all at once (their extent look-ups are chains of dependent loads: one after the other they cost
    // a memory round trip per round), then the rounds from LDS
    __shared__ int c_x[kPlanChunk][kPlanLanes], c_y[kPlanChunk][kPlanLanes];
    const int r_begin = chunk * kPlanChunk, r_end = min(head, (chunk + 1) * kPlanChunk);
    const bool valid = lane < nlb;
#pragma unroll
    for (int i = 0; i < kPlanChunk; ++i)
        if (valid && r_begin + i < r_end) {
            const int2 en = plan_tile_entry(L, s_first, xcd, (r_begin + i) * nlb + lane);
            c_x[i][lane] = en.x; c_y[i][lane] = en.y;
        }
    for (int r = r_begin; r < r_end; ++r) {
        const int2 en = valid ? make_int2(c_x[r - r_begin][lane], c_y[r - r_begin][lane]) : make_int2(0, 0);
        const int cst = valid ? (en.y & 0xFFFF) + L.fixed : -1;
        const int mine = s_load[lane];
        s_cost[lane] = cst;
        __syncthreads();
        int crank = 0, lrank = 0;                          // longest tile first; least-loaded workgroup first (ties: by index)
        for (int k = 0; k < nlb; ++k) {
            const int ck = s_cost[k], lk = s_load[k];
            crank += (ck > cst || (ck == cst && k < lane)) ? 1 : 0;
            lrank += (lk < mine || (lk == mine && k < lane)) ? 1 : 0;
        }
        if (valid) s_who[lrank] = lane;
        __syncthreads();
        if (valid) {
            const int w = s_who[crank];
            L.plan[((int64_t)xcd * nlb + w) * L.rounds + r] = en;
            s_load[w] += cst * plan_weight(L, s_bias3, nlb, w);
        }
        __syncthreads();
    }
    if (chunk != n_chunks - 1) return;
    // ---- the rest as one batch, by the block that dealt the last chunk (on top of that chunk's loads)
    const int t0 = head * nlb, n_tail = n_tiles - t0;
    for (int i = lane; i < n_tail; i += kPlanLanes) {
        const int2 en = plan_tile_entry(L, s_first, xcd, t0 + i);
        t_cost[i] = (en.y & 0xFFFF) + L.fixed;
        t_x[i] = en.x;
        t_y[i] = en.y;
    }
    __syncthreads();
    for (int i = lane; i < n_tail; i += kPlanLanes) {
        const int c = t_cost[i];
        int rank = 0;
        for (int j = 0; j < n_tail; ++j) rank += (t_cost[j] > c || (t_cost[j] == c && j < i)) ? 1 : 0;
        t_by_rank[rank] = i;
    }
    __syncthreads();
    // each item, longest first, to the workgroup with the least load at that moment: a serial loop, run by the first wave alone
    // (shuffles, no block barrier), lane j looking after workgroups j and j + 64
    if (lane >= 64) return;
    const int wg[2] = {lane, lane + 64};
    int pos[2] = {head, head};
    unsigned load[2] = {(unsigned)s_load[wg[0]], (unsigned)s_load[wg[1]]};
    int wt[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) wt[h] = plan_weight(L, s_bias3, nlb, wg[h]);
    for (int q = 0; q < n_tail; ++q) {
        const int item = t_by_rank[q];
        unsigned key = 0xFFFFFFFFu;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (wg[h] < nlb && pos[h] < L.rounds) key = min(key, (min(load[h], 0x00FFFFFFu) << 7) | (unsigned)wg[h]);
        for (int off = 32; off > 0; off >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, off));
        if (key == 0xFFFFFFFFu) break;                      // (no list has room: cannot happen, the lists have kPlanSlack spare entries)
        const int w = (int)(key & 127u);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (w == wg[h]) {
                L.plan[((int64_t)xcd * nlb + w) * L.rounds + pos[h]++] = make_int2(t_x[item], t_y[item]);
                load[h] += (unsigned)(t_cost[item] * wt[h]);
            }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (wg[h] < nlb)
            for (; pos[h] < L.rounds; ++pos[h]) L.plan[((int64_t)xcd * nlb + wg[h]) * L.rounds + pos[h]] = make_int2(0, 0);
}

hipError_t launch_tile_plan(const PlanLaunch* d_launches, int n_launches, int max_rounds, hipStream_t stream) {
    if (n_launches <= 0) return hipSuccess;
    (void)hipGetLastError();
    const int chunks = std::max(1, (std::max(0, max_rounds - kPlanSlack - kPlanTail) + kPlanChunk - 1) / kPlanChunk);
    hipLaunchKernelGGL(tile_plan_kernel, dim3(8, n_launches, chunks), dim3(kPlanLanes), 0, stream, d_launches);
    return hipGetLastError();
}

}  // namespace cafe
