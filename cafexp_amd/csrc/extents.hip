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

__global__ __launch_bounds__(kBN) void node_extent_kernel(const ExtArgs a) {
    const ExtNode& nd = a.nodes[a.first + blockIdx.z];
    const int col = blockIdx.x * kBN + threadIdx.x;
    if (blockIdx.x * kBN >= nd.cols) return;               // (levels are launched as wide as their widest node)
    const int k = blockIdx.y;
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
            const int32_t* e = a.kext + (int64_t)(k * a.n_pairs_inner + nd.inner_pair[j]) * a.kext_blocks * 2;
            for (int b = 0; b < a.kext_blocks; ++b)
                if (e[2 * b + 1] >= clo && e[2 * b] <= chi) { flo = min(flo, 16 * b + 1); fhi = max(fhi, 16 * b + 16); }
            if (clo == 0) { flo = 0; fhi = max(fhi, 0); }
            fhi = min(fhi, a.M);
        }
        lo = max(lo, flo); hi = min(hi, fhi);
    }
    if (hi < lo) { lo = 0x7fffffff; hi = -1; }
    int32_t* out = nd.colext + ((int64_t)k * nd.cols + col) * 2;
    out[0] = lo; out[1] = hi;
    // hull over the 128 columns of the tile
    __shared__ int s_lo[2], s_hi[2];
    for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_down(lo, off)); hi = max(hi, __shfl_down(hi, off)); }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t* t = nd.tileext + ((int64_t)k * (nd.cols / kBN) + blockIdx.x) * 2;
        t[0] = min(s_lo[0], s_lo[1]); t[1] = max(s_hi[0], s_hi[1]);
    }
}

hipError_t launch_node_extents(const ExtArgs& a, int max_col_tiles, int n_categories, hipStream_t stream) {
    if (a.count <= 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(node_extent_kernel, dim3(max_col_tiles, n_categories, a.count), dim3(kBN), 0, stream, a);
    return hipGetLastError();
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

// one workgroup per (k-step, k-major slot): the four matrix rows c = 4 ks .. 4 ks + 3 over all parent sizes
__global__ __launch_bounds__(256) void mag_kmajor_kernel(const MagArgs a) {
    __shared__ double s_max[2048], s_sum[2048];
    const int ks = blockIdx.x, slot = blockIdx.y, tid = threadIdx.x;
    const int ncol = min(a.kpool.n - 1, 2048);             // parent sizes 1 .. n - 1 are columns 0 .. n - 2
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

// one workgroup per (row step, row-major slot): rows s = 4 r .. 4 r + 3 over the counts x <= M
__global__ __launch_bounds__(256) void mag_leaf_kernel(const MagArgs a) {
    const int r = blockIdx.x, slot = blockIdx.y;
    const double* P = a.lpool.base + (int64_t)slot * a.lpool.stride;
    for (int x = threadIdx.x; x <= a.M && x < a.lpool.n; x += 256) {
        double mx = (r == 0 && x == 0) ? 1.0 : 0.0;
        for (int s = 4 * r; s < 4 * r + 4 && s < a.lpool.n; ++s) mx = fmax(mx, P[(int64_t)s * a.lpool.ld + x]);
        a.lt[((int64_t)slot * (a.M + 1) + x) * a.n_rsteps + r] = mag_of(mx);
    }
}

hipError_t launch_magnitude_tables(const MagArgs& a, hipStream_t stream) {
    (void)hipGetLastError();
    if (a.n_kslots > 0) hipLaunchKernelGGL(mag_kmajor_kernel, dim3(a.n_ksteps, a.n_kslots), dim3(256), 0, stream, a);
    if (a.n_lslots > 0) hipLaunchKernelGGL(mag_leaf_kernel, dim3(a.n_rsteps, a.n_lslots), dim3(256), 0, stream, a);
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
// The loops over counts, child tiles and k-steps read tables far larger than the caches: each batches kBoundBatch independent
// loads in front of the arithmetic (one after the other they cost a memory round trip per item: 7.3 ms per bench call).
constexpr int kBoundThreads = 256, kBoundBatch = 16;
__global__ __launch_bounds__(kBoundThreads) void node_bound_kernel(const ExtArgs a) {
    const ExtNode& nd = a.nodes[a.first + blockIdx.z];
    if (blockIdx.x * kBN >= nd.cols) return;
    const int k = blockIdx.y, ct = blockIdx.x, tid = threadIdx.x, col = ct * kBN + (tid & (kBN - 1));
    const int nr = a.n_rsteps, nk = a.n_ksteps, nct = nd.cols / kBN;
    __shared__ int32_t s_acc[kMaxSteps], s_cb[kMaxSteps];
    __shared__ int s_list[kBN];                            // the distinct counts / child tiles of the tile's columns
    __shared__ unsigned s_bits[kMaxSteps / 8];             // counts 0 .. 2047
    __shared__ int s_n, s_klo, s_khi;
    for (int r = tid; r < nr; r += kBoundThreads) s_acc[r] = 0;
    for (int l = 0; l < nd.n_leaf; ++l) {
        __syncthreads();
        if (tid < kMaxSteps / 8) s_bits[tid] = 0;
        if (tid == 0) s_n = 0;
        __syncthreads();
        if (tid < kBN) {
            const int x = nd.cnt[(int64_t)nd.leaf_row[l] * nd.cnt_ld + col];
            if (!(atomicOr(&s_bits[x >> 5], 1u << (x & 31)) & (1u << (x & 31)))) s_list[atomicAdd(&s_n, 1)] = x;    // the first to set it
        }
        __syncthreads();
        const int n = s_n;
        const int32_t* lt = a.lt + (int64_t)(k * a.n_pairs_leaf + nd.leaf_pair[l]) * (a.M + 1) * nr;
        for (int r = tid; r < nr; r += kBoundThreads) {
            int32_t m = kMagNone;
            for (int i0 = 0; i0 < n; i0 += kBoundBatch) {
                int32_t v[kBoundBatch];
#pragma unroll
                for (int i = 0; i < kBoundBatch; ++i) v[i] = lt[(int64_t)s_list[min(i0 + i, n - 1)] * nr + r];
#pragma unroll
                for (int i = 0; i < kBoundBatch; ++i) m = max(m, v[i]);
            }
            s_acc[r] = (m == kMagNone || s_acc[r] == kMagNone) ? kMagNone : s_acc[r] + m;
        }
    }
    for (int j = 0; j < nd.n_inner; ++j) {
        __syncthreads();
        if (tid < kMaxSteps / 8) s_bits[tid] = 0;
        if (tid == 0) { s_n = 0; s_klo = nk; s_khi = -1; }
        __syncthreads();
        if (tid < kBN) {
            const int t = (nd.inner_map[j] ? nd.inner_map[j][col] : col) / kBN;
            // (tiles past the bitmap enter the list once per column: that costs loads and changes no maximum)
            if (t >= kMaxSteps * 4 || !(atomicOr(&s_bits[t >> 5], 1u << (t & 31)) & (1u << (t & 31)))) s_list[atomicAdd(&s_n, 1)] = t;
        }
        __syncthreads();
        const int n = s_n;
        const int32_t* cb = nd.inner_bound[j] + (int64_t)k * (nd.inner_cols[j] / kBN) * nr;
        for (int ks = tid; ks < nk; ks += kBoundThreads) {
            int32_t m = kMagNone;
            for (int i0 = 0; i0 < n; i0 += kBoundBatch) {
                int32_t v[kBoundBatch];
#pragma unroll
                for (int i = 0; i < kBoundBatch; ++i) v[i] = cb[(int64_t)s_list[min(i0 + i, n - 1)] * nr + ks];
#pragma unroll
                for (int i = 0; i < kBoundBatch; ++i) m = max(m, v[i]);
            }
            s_cb[ks] = m;
            if (m != kMagNone) { atomicMin(&s_klo, ks); atomicMax(&s_khi, ks); }
        }
        __syncthreads();
        const int slot = k * a.n_pairs_inner + nd.inner_pair[j];
        const int32_t* t4 = a.t4 + (int64_t)slot * nk * nr;
        const int32_t* e = a.kext + (int64_t)slot * a.kext_blocks * 2;
        for (int r = tid; r < nr; r += kBoundThreads) {
            // the k-steps inside the child's support and inside the non-zero extents of the matrix blocks that hold the parent
            // sizes 4 r .. 4 r + 3 (block b: sizes 16 b + 1 .. 16 b + 16; size 0 only reaches child size 0)
            int klo = nk, khi = -1;
            for (int b = max(4 * r - 1, 0) / 16; b <= (4 * r + 2) / 16 && b < a.kext_blocks; ++b)
                if (e[2 * b + 1] >= e[2 * b]) { klo = min(klo, e[2 * b] / 4); khi = max(khi, e[2 * b + 1] / 4); }
            if (r == 0) klo = 0, khi = max(khi, 0);
            klo = max(klo, s_klo); khi = min(min(khi, s_khi), nk - 1);
            int32_t top = kMagNone;                         // running maximum and sum_i 2^(v_i - top)
            float sum = 0.f;
            for (int k0 = klo; k0 <= khi; k0 += kBoundBatch) {
                int32_t tv[kBoundBatch];
#pragma unroll
                for (int i = 0; i < kBoundBatch; ++i) tv[i] = t4[(int64_t)min(k0 + i, khi) * nr + r];
#pragma unroll
                for (int i = 0; i < kBoundBatch; ++i) {
                    const int32_t cv = s_cb[min(k0 + i, khi)];
                    if (k0 + i > khi || tv[i] == kMagNone || cv == kMagNone) continue;
                    const int32_t v = tv[i] + cv;
                    if (v > top) { sum = sum * exp2f((float)(top - v) * (1.f / kMagUnit)) + 1.f; top = v; }
                    else sum += exp2f((float)(v - top) * (1.f / kMagUnit));
                }
            }
            const int32_t f = top == kMagNone ? kMagNone : top + (int32_t)ceilf(log2f(sum) * (float)kMagUnit) + 1;
            s_acc[r] = (f == kMagNone || s_acc[r] == kMagNone) ? kMagNone : s_acc[r] + f;
        }
    }
    __syncthreads();
    const int32_t* te = nd.tileext + ((int64_t)k * nct + ct) * 2;
    const int lo = te[0], hi = te[1];
    int32_t* out = nd.bound + ((int64_t)k * nct + ct) * nr;
    for (int r = tid; r < nr; r += kBoundThreads)
        out[r] = (hi >= lo && 4 * r + 3 >= lo && 4 * r <= hi) ? max(s_acc[r], kMagFloor) + kMagSlack : kMagNone;
}

hipError_t launch_node_bounds(const ExtArgs& a, int max_col_tiles, int n_categories, hipStream_t stream) {
    if (a.count <= 0 || !a.t4) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(node_bound_kernel, dim3(max_col_tiles, n_categories, a.count), dim3(kBoundThreads), 0, stream, a);
    return hipGetLastError();
}

// Joint K ranges (GemmOp::jr): lane = 16-row block of the op's matrix.  The exact interval is the block's matrix extent cut
// by the panel's (an empty panel extent: row 0, so that the panel receives its zeros); with magnitude tables the interval
// shrinks from both ends while (largest entry of the block in the k-step) x (bound of the panel's rows of the k-step) lies
// below 2^-1100.  The ranges only ever shrink: no MFMA reads a panel row the assemble pass left unwritten.
__global__ __launch_bounds__(256) void range_kernel(const RangeArgs a) {
    const GemmOp& o = a.ops[blockIdx.z];
    if (!o.jr || (int)blockIdx.x >= o.jr_nct) return;
    const int ct = blockIdx.x, cat = blockIdx.y, b = threadIdx.x, nb = a.ext_blocks;
    const bool mag = a.a16 && o.bbound;
    __shared__ int32_t s_b[kMaxSteps];                      // the panel's bound per k-step
    if (mag) {
        const int32_t* B = o.bbound + ((int64_t)cat * o.jr_nct + ct) * a.n_rsteps;
        for (int i = b; i < a.n_ksteps; i += 256) s_b[i] = B[i];
        __syncthreads();
    }
    if (b >= nb + kRangePad) return;
    int slo = 1, shi = 0;
    if (b < nb) {
        const int slot = o.slot[cat];
        const int32_t* e = a.aext + ((int64_t)slot * nb + b) * 2;
        int plo = 0, phi = a.k_valid - 1;
        if (o.bext) {
            const int32_t* be = o.bext + ((int64_t)cat * o.jr_nct + ct) * 2;
            plo = be[0]; phi = min(be[1], phi);
            if (be[1] < be[0]) { plo = 0; phi = 0; }
        }
        const int lo = max(e[0], plo), hi = min(e[1], phi);
        if (hi >= lo) {
            slo = lo / 4; shi = hi / 4;
            if (mag) {
                // four k-steps per look from either end (independent loads); a step counts when it may reach 2^-1100
                const int32_t* A = a.a16 + (int64_t)slot * a.n_ksteps * nb + b;
                const int first = slo, last = shi;
                for (bool found = false; !found && slo <= last; ) {
                    int32_t v[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = A[(int64_t)min(slo + i, last) * nb];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (!found) { if (slo <= last && v[i] + s_b[slo] >= kSkipBelow) found = true; else ++slo; }
                }
                for (bool found = false; !found && shi >= slo; ) {
                    int32_t v[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = A[(int64_t)max(shi - i, first) * nb];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (!found) { if (shi >= slo && v[i] + s_b[shi] >= kSkipBelow) found = true; else --shi; }
                }
                if (slo > shi) { slo = 1; shi = 0; }
            }
        }
    }
    const_cast<int32_t*>(o.jr)[((int64_t)cat * o.jr_nct + ct) * (nb + kRangePad) + b] = slo | (shi << 16);
}

hipError_t launch_joint_ranges(const RangeArgs& a, int max_col_tiles, int n_categories, hipStream_t stream) {
    if (a.n_ops <= 0 || !a.aext) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(range_kernel, dim3(max_col_tiles, n_categories, a.n_ops), dim3(256), 0, stream, a);
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
__device__ inline int plan_weight(const PlanLaunch& L, int nlb, int w) {
    if (nlb == 64 && L.bias) return w < 32 ? 100 - L.bias : 100 + L.bias;
    if (nlb == 96 || nlb == 128) return L.bias3[w >> 5];
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
    __shared__ int s_first[kMaxGroupOps + 1];
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
            s_load[w] += cst * plan_weight(L, nlb, w);
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
    for (int h = 0; h < 2; ++h) wt[h] = plan_weight(L, nlb, wg[h]);
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
