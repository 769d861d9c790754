// The per-level kernel of the extent pass (extents.hip has the reasoning): the interval of a panel column, the magnitude of a
// value, and node_level_kernel, a template on MISSING -- whether a count may be CAFE_COUNT_MISSING.  extents.hip instantiates
// MISSING = false, the kernel every context without a missing cell runs; extents_missing.hip instantiates MISSING = true and
// holds its launcher.  One instantiation per translation unit, like the slot types of K1 and of the per-family kernel.
#pragma once

#include "cafe_kernels.h"

namespace cafe {

// the interval of one panel column (node_level_kernel below runs it per column and reduces a tile's hull).  kext: the extents
// of the interior children's matrices, staged in LDS by the caller -- every column walks all their blocks, and from global
// memory each step of that walk is a dependent load.  mono[j]: first and last child size of child j's matrix do not decrease
// from block to block (a band: the caller checks it) -- the blocks that meet a child interval are then the run between
// the first block whose last size reaches the interval and the last block whose first size does, found by two binary
// searches instead of the walk; the same blocks, so the same interval.  Any other matrix takes the walk.
// MISSING: a count may be CAFE_COUNT_MISSING (cafe_kernels.h).  Such a leaf's factor is 1.0 in every row: it narrows no interval.
constexpr int kMaxExtBlocks = 128;                         // blocks of 16 parent sizes of the largest matrix order (2048)
template <bool MISSING>
__device__ inline int2 column_interval(const ExtArgs& a, const ExtNode& nd, int k, int col, const int32_t (*kext)[2 * kMaxExtBlocks],
                                       const int* mono) {
    int lo = 0, hi = a.M;
    const int half = a.n_dev > 0 ? (a.n_dev - 1) / 2 : 0;
    for (int l = 0; l < nd.n_leaf; ++l) {
        const int x = nd.cnt[(int64_t)nd.leaf_row[l] * nd.cnt_ld + col];
        if (MISSING && count_is_missing(x)) continue;
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

// upper bound of log2(v) in 1/256, v >= 0
__device__ inline int32_t mag_of(double v) {
    if (!(v > 0.0)) return kMagNone;
    int e;
    const double m = frexp(v, &e);                         // v = m 2^e, m in [0.5, 1)
    return e * kMagUnit + (int32_t)ceilf(log2f((float)m) * (float)kMagUnit) + 1;
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
// MISSING: a count may be CAFE_COUNT_MISSING.  A missing leaf narrows no interval (column_interval) and its factor, exactly
// 1.0 in every row, is bounded by kMagOne: a tile's leaf bound is the largest over the counts that occur in it AND, when one
// of its columns is missing, kMagOne -- it still dominates every computed entry of the tile.
constexpr int32_t kMagOne = 1;                             // mag_of(1.0): log2 = 0, rounded up by the unit mag_of adds
template <bool MISSING>
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
    // One buffer, two lives inside an interior child's turn: first the narrowed interval of each listed child tile, in k-steps
    // (read while the child's bounds are gathered), then, from the barrier behind that gather on, the partial sums' maxima.
    // Keeping them apart would put the workgroup over a fifth of a CU's LDS.
    __shared__ union {
        int32_t ptop[kLevelPhases][kLevelTiles][64];
        struct { int lo[kLevelTiles][kBN], hi[kLevelTiles][kBN]; } child;
    } s_u;
    __shared__ float s_psum[kLevelPhases][kLevelTiles][64];
    __shared__ int32_t s_kext[kMaxExtChildren][2 * kMaxExtBlocks];     // the interior children's matrix extents (this category)
    __shared__ int s_mono[kMaxExtChildren];                // the child's matrix extents do not decrease from block to block
    __shared__ int s_miss[MISSING ? kLevelTiles : 1];      // MISSING: some column of the tile has no count for the leaf at hand
    __shared__ int s_nlo[kLevelTiles], s_nhi[kLevelTiles];  // first / last row step of a tile that is not proven zero
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
        if (tid + p * kLevelThreads < nt * kBN) iv[p] = column_interval<MISSING>(a, nd, k, ct0 * kBN + tid + p * kLevelThreads, s_kext, s_mono);
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
        if (!a.t4 || !a.narrow) {                           // no bounds to cut by: the narrowed interval is the hull
            int32_t* n = nd.narrow + ((int64_t)k * nct + ct0 + tid) * 2;
            n[0] = lo; n[1] = hi;
        }
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
        if (tid < kLevelTiles) { s_n[tid] = 0; if (MISSING) s_miss[tid] = 0; }
        __syncthreads();
        for (int i = tid; i < nt * kBN; i += kLevelThreads) {
            const int c = i / kBN;
            const int x = nd.cnt[(int64_t)nd.leaf_row[l] * nd.cnt_ld + ct0 * kBN + i];
            if (MISSING && count_is_missing(x)) { s_miss[c] = 1; continue; }      // (every writer stores the same value)
            if (!(atomicOr(&s_bits[c][x >> 5], 1u << (x & 31)) & (1u << (x & 31)))) s_list[c][atomicAdd(&s_n[c], 1)] = x;    // the first to set it
        }
        __syncthreads();
        const int32_t* lt = a.lt + (int64_t)(k * a.n_pairs_leaf + nd.leaf_pair[l]) * (a.M + 1) * nr;
        const int span = rhi - rlo + 1;
        for (int i = tid; i < nt * span; i += kLevelThreads) {
            const int c = i / span, r = rlo + i % span;
            if (r < s_rlo[c] || r > s_rhi[c]) continue;
            const int n = s_n[c];
            int32_t m = (MISSING && s_miss[c]) ? kMagOne : kMagNone;
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
        // (a child tile's rows outside its narrowed interval are computed zeros: their bound counts as "none" here, whatever
        // floor the table holds -- what is cut at one level shortens the sums of the next)
        if (a.narrow) {
            const int32_t* cn = nd.inner_narrow[j] + (int64_t)k * (nd.inner_cols[j] / kBN) * 2;
            for (int i = tid; i < nt * kBN; i += kLevelThreads) {
                const int c = i / kBN, q = i % kBN;
                if (q >= s_n[c]) continue;
                const int lo = cn[2 * s_list[c][q]], hi = cn[2 * s_list[c][q] + 1];
                s_u.child.lo[c][q] = hi >= lo ? lo / 4 : nk; s_u.child.hi[c][q] = hi >= lo ? hi / 4 : -1;
            }
            __syncthreads();
        }
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
                if (a.narrow) {
#pragma unroll
                    for (int q = 0; q < kListBatch; ++q)
                        if (ks < s_u.child.lo[c][min(i0 + q, n - 1)] || ks > s_u.child.hi[c][min(i0 + q, n - 1)]) v[q] = kMagNone;
                }
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
            for (int c = 0; c < kLevelTiles; ++c) { s_u.ptop[wave][c][lane] = top[c]; s_psum[wave][c][lane] = sum[c]; }
            __syncthreads();
            {   // thread -> (tile, row step of the chunk): the partial sums in the order of the waves
                const int c = wave, rr = r0 + lane;
                if (c < nt && rr >= s_rlo[c] && rr <= s_rhi[c]) {
                    int32_t T = kMagNone;
#pragma unroll
                    for (int w = 0; w < kLevelPhases; ++w) T = max(T, s_u.ptop[w][c][lane]);
                    int32_t f = kMagNone;
                    if (T != kMagNone) {
                        float S = 0.f;
#pragma unroll
                        for (int w = 0; w < kLevelPhases; ++w)
                            if (s_u.ptop[w][c][lane] != kMagNone) S += s_psum[w][c][lane] * exp2f((float)(s_u.ptop[w][c][lane] - T) * (1.f / kMagUnit));
                        f = T + (int32_t)ceilf(log2f(S * (1.f + 0x1p-11f)) * (float)kMagUnit);
                        // (a factor whose whole sum is below 2^-1100 is a computed zero, whatever its siblings hold: every
                        // product that feeds it rounds to zero.  "None" makes the row step one that the narrowing may cut.)
                        if (a.narrow && f < kSkipBelow) f = kMagNone;
                    }
                    s_acc[c][rr] = (f == kMagNone || s_acc[c][rr] == kMagNone) ? kMagNone : s_acc[c][rr] + f;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (a.narrow) {
        // ---- the narrowed interval: the hull cut back from both ends over the row steps whose bound, before the floor, lies
        // below kSkipBelow (cafe_kernels.h: computed zeros only).  Row steps between two that count are never dropped.
        // (K2 copies row 0 of a child's panel outside any K range.  A hull that holds row 0 keeps it: a column's interval
        // reaches row 0 only where every leaf below is 0 or missing, that column's row 0 is exactly 1, and a bound that
        // dominates it is far above the threshold.  A hull that does not hold row 0 had that row written by the assemble pass
        // only while it began below row 16; cut back to row 16 or beyond, it now leaves row 0 as it was -- as every hull that
        // begins there structurally always did.  What stands there is what an earlier call wrote, and without an error model a
        // column's row 0 is the same in every call: 1 where every leaf below is 0 or missing, else exactly 0, whatever the
        // rates.  An error model's taps make it non-zero only in a column with a count of 1, whose rows 1 .. 3 are then far
        // above the threshold in a call without the model: row step 0 is kept and row 0 rewritten.)
        if (tid < kLevelTiles) { s_nlo[tid] = nr; s_nhi[tid] = -1; }
        __syncthreads();
        for (int i = tid; i < nt * nr; i += kLevelThreads) {
            const int c = i / nr, r = i % nr;
            if (r >= s_rlo[c] && r <= s_rhi[c] && s_acc[c][r] + kMagSlack >= kSkipBelow) { atomicMin(&s_nlo[c], r); atomicMax(&s_nhi[c], r); }
        }
        __syncthreads();
        if (tid < nt) {
            const bool some = s_nhi[tid] >= s_nlo[tid];
            int32_t* n = nd.narrow + ((int64_t)k * nct + ct0 + tid) * 2;
            n[0] = some ? max(s_lo[tid], 4 * s_nlo[tid]) : 0x7fffffff; n[1] = some ? min(s_hi[tid], 4 * s_nhi[tid] + 3) : -1;
        }
    }
    for (int i = tid; i < nt * nr; i += kLevelThreads) {
        const int c = i / nr, r = i % nr, lo = s_lo[c], hi = s_hi[c];
        nd.bound[((int64_t)k * nct + ct0 + c) * nr + r] =
            (hi >= lo && 4 * r + 3 >= lo && 4 * r <= hi) ? max(s_acc[c][r], kMagFloor) + kMagSlack : kMagNone;
    }
}

// the MISSING = true instantiation (extents_missing.hip): the grid and the tiles per workgroup are launch_node_level's
hipError_t launch_node_level_missing(const ExtArgs& a, dim3 grid, int per_block, hipStream_t stream);

}  // namespace cafe
