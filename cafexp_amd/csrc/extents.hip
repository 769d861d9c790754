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

#include "extents_level.h"

namespace cafe {

// ---- Magnitudes: K steps whose products underflow below the smallest denormal.
// The extents above leave out a product only when one factor is exactly zero.  A product of two non-zero factors below
// 2^-1075 has no effect either: all operands are non-negative, an accumulator that is 0 stays 0 and one that is not is at
// least 2^-1074 and does not move under round-to-nearest, whether the MFMA fuses its four products, chains them or rounds
// each one.  Three steps, all per call: (1) tables of the largest entries of this call's matrices, one pass over the pools;
// (2) upper bounds of the panels, propagated with the intervals, level by level; (3) per (op, category, column tile,
// 16-row block) the k-steps that can still matter, cut out of the exact interval.

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

// Tiles a workgroup owns (ExtArgs::level_tiles, or 0: chosen here): four where that still leaves the level's grid ten
// workgroups per CU's worth of tiles, two from five (five are resident per CU; with fewer tiles one workgroup each keeps
// more CUs busy).  A tile's bound does not depend on the choice (node_level_kernel: the grid of its rounds is absolute).
hipError_t launch_node_level(const ExtArgs& a, int max_col_tiles, int n_categories, hipStream_t stream, bool missing) {
    if (a.count <= 0) return hipSuccess;
    const int64_t tiles = (int64_t)max_col_tiles * n_categories * a.count, cus = std::max(1, a.n_cu);
    int per_block = !a.t4 ? 2 : tiles >= 10 * cus ? kLevelTiles : tiles >= 5 * cus ? 2 : 1;
    if (a.level_tiles == 1 || a.level_tiles == 2 || a.level_tiles == kLevelTiles) per_block = a.level_tiles;
    (void)hipGetLastError();
    const dim3 grid((max_col_tiles + per_block - 1) / per_block, n_categories, a.count);
    if (missing) return launch_node_level_missing(a, grid, per_block, stream);      // (extents_missing.hip)
    hipLaunchKernelGGL(node_level_kernel<false>, grid, dim3(kLevelThreads), 0, stream, a, per_block);
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
    // with magnitude tables the panel's extent is its narrowed hull (ExtNode::narrow): the rows outside it are computed zeros,
    // their bound counts as "none" whatever floor the table holds, and the assemble passes do not write them
    const int32_t* pext = mag && o.bnarrow ? o.bnarrow : o.bext;
    if (mag) {
        if (live) {
            const int32_t* B = o.bbound + ((int64_t)cat * o.jr_nct + ct) * a.n_rsteps;
            int nlo = 0, nhi = a.n_ksteps - 1;
            if (o.bnarrow) {
                const int32_t* be = o.bnarrow + ((int64_t)cat * o.jr_nct + ct) * 2;
                nlo = be[1] >= be[0] ? be[0] / 4 : a.n_ksteps; nhi = be[1] >= be[0] ? be[1] / 4 : -1;
            }
            for (int i = lane; i < a.n_ksteps; i += 64) s_ball[wave][i] = (i >= nlo && i <= nhi) ? B[i] : kMagNone;
        }
        __syncthreads();
    }
    if (!live) return;
    const int slot = o.slot[cat];
    int plo = 0, phi = a.k_valid - 1;
    if (pext) {
        const int32_t* be = pext + ((int64_t)cat * o.jr_nct + ct) * 2;
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
        // An all-zero tile still runs one K tile: the panel must receive its zeros.  zlo stays the STRUCTURAL first row, not
        // the narrowed one: the K tile there is fetched and never multiplied (every block's mask is empty), so it may hold rows
        // that a narrowed assemble pass left as an earlier call wrote them -- finite, the panels are cleared after a call that
        // returned NaN -- and the entry stays what cafe_debug_plan_check and the tests of the lists recompute.
        if (shi < slo) { lo = zlo; hi = zlo; }
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
