// Device-side interface of the MI355X likelihood path: argument blocks and launchers of
// the four kernels:
//   K1 bd_matrix_build  -- replaces matrix_cache::precalculate_matrices (matrix_cache.cpp:121)
//   K2 prune_gemm       -- replaces matrix::multiply for interior children (matrix_cache.cpp:28)
//   K3 leaf_gather      -- replaces the leaf branch of compute_node_probability (probability.cpp:179)
//   K4 root_reduce      -- replaces the per-family loops of base_model.cpp:89 / gamma_core.cpp:144
// gfx950 only; no other target is supported or tested.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace cafe {

constexpr int kMaxCategories = 32;   // CAFE_MAX_CATEGORIES
constexpr int kMaxLeafPerOp = 4;     // leaf children folded by one gather launch / one GEMM epilogue

// Missing cells (CAFE_COUNT_MISSING, include/cafe_mi355x.h): THE rule, for every kernel that turns a leaf count into a factor.
// A missing leaf's factor is exactly 1.0 for every parent size -- no matrix column, no error-model taps.  A reader keeps its
// addresses in bounds with count_index (column 0 stands in for the load whose value is then dropped) and takes its factor
// through leaf_factor_or_one; a product with 1.0 leaves every bit of the other factors as it is, so the value is that of the
// tree without the leaf.  Only the MISSING instantiations of the readers call these: contexts without a missing cell run the
// code they ran before.
__host__ __device__ inline bool count_is_missing(int x) { return x < 0; }
__host__ __device__ inline int count_index(int x) { return x < 0 ? 0 : x; }
__host__ __device__ inline double leaf_factor_or_one(int x, double fac) { return x < 0 ? 1.0 : fac; }

// GEMM tiling (fp64 MFMA 16x16x4): block tile (16*MI) x 128, K step 16, 4 waves side by side in N
constexpr int kBN = 128;
constexpr int kBK = 16;          // largest depth of a K tile (panel / matrix row counts are rounded to it); a context runs K2 with 16-deep
                                 // K tiles (small matrices: a launch is one round of tiles, fewer DMA round trips per tile), 8-deep ones
                                 // (half the LDS per stage: four workgroups per CU) or 12-deep ones (still four: 39 936 bytes each, a
                                 // third fewer barriers per MFMA) -- GemmArgs::kb.  A 12-deep last K tile may stage rows past the
                                 // rounded count: the buffer descriptors end at the matrix / the panel category, the DMA reads zeros or
                                 // the neighbour's rows there, and no MFMA uses them (only k-steps with a valid k run)
constexpr int kMaxBM = 144;          // largest row tile (MI = 9)

// Per transition matrix: a = lambda_q t_q / (1 + lambda_q t_q) of the de-quantized key
// (matrix_cache.cpp:148-149), oma2 = (1-a)^2; zero = saturated (matrix_cache.cpp:153) or
// !(coeff > 0 && coeff != 1) (probability.cpp:154): rows s >= 1 stay 0.
struct SlotParam {
    static constexpr bool two_rates = false;
    double alpha;
    double oma2;
    int32_t zero;
    int32_t pad;
};

// The matrices of a call live in two pools, slot i at base + i*stride (bd_matrix.hip):
//   row-major (kmajor = 0): P[s][c], n rows, leading dimension ld (multiple of 16), columns >= n zero;
//   k-major   (kmajor = 1): Pt[c][j] = P[j+1][c], `rows` rows (round_up(M+1, kBK); rows >= k_valid = M+1
//                           are zero), leading dimension ld >= n-1 + one row tile, columns >= n-1 zero.
struct MatrixPool {
    double* base;
    int64_t stride;
    int32_t ld;
    int32_t n;        // matrix order N = max(M,R)+1
    int32_t rows;     // k-major: rows written
    int32_t k_valid;  // k-major: M+1
    int32_t kmajor;
    // k-major only: per matrix and per block of 16 consecutive parent sizes (columns of Pt), the first and last
    // contraction index c whose entries are not all exactly 0 -- ext[(slot * ext_blocks + block) * 2 + {0, 1}], written by
    // K1 (first > last: the block is all zero).  Far from the diagonal the entries of a short branch underflow to exact
    // zeros; K2 skips the K tiles that lie outside a row tile's extent (adding exact zeros changes no bit).
    int32_t* ext;
    int32_t ext_blocks;
};

// The reference keeps a matrix under the key (long(lambda * 1e9), long(t * 1000)) (matrix_cache_key, matrix_cache.h:42-61)
// and builds it from the DE-QUANTIZED key (precalculate_matrices, matrix_cache.cpp:148-153).  Every entry point builds
// its slot parameters through these three, so that they agree with the reference, and with each other, to the bit.
// A lambda * 1e9 beyond a long is the caller's to reject or to treat (family_lambda.hip).
inline long quantize_lambda(double lambda) { return long(lambda * 1000000000); }
inline long quantize_time(double t) { return long(t * 1000); }
inline SlotParam slot_param(long lq, long tq) {
    const double lambda_q = double(lq) / 1000000000.0, t_q = double(tq) / 1000.0;
    const double alpha = lambda_q * t_q / (1 + lambda_q * t_q), coeff = 1 - 2 * alpha;
    SlotParam sp;
    sp.alpha = alpha;
    sp.oma2 = (1 - alpha) * (1 - alpha);
    sp.zero = !(coeff > 0 && coeff != 1);       // saturated (coeff < 0) or degenerate: rows s >= 1 are 0
    sp.pad = 0;
    return sp;
}
// Separate birth and death rates (bd_row.h).  The single-lineage law of the linear birth-death process is
// p1(0) = alpha, p1(k) = (1-alpha)(1-beta) beta^(k-1),
//     alpha = mu (E-1) / (lambda E - mu),   beta = lambda (E-1) / (lambda E - mu),   E = exp((lambda - mu) t).
// Evaluated as w = -expm1(-|lambda-mu| t), D = |lambda-mu| + min(lambda, mu) w, alpha = mu w / D, beta = lambda w / D: every
// term is non-negative, nothing overflows however large |lambda-mu| t is, and both tend to lambda t / (1 + lambda t) as
// mu -> lambda.  Equal rates take that formula itself, so that alpha has slot_param's bits.  Mathematically alpha, beta < 1;
// a quotient that rounds up to 1 is put back to the largest double below it.  Plain doubles in, no quantization.
struct BdRates { double alpha, beta, coeff; };
inline BdRates bd_rates(double lambda, double mu, double t) {
    BdRates r;
    if (lambda == mu) {
        r.alpha = r.beta = lambda * t / (1 + lambda * t);
        r.coeff = 1 - 2 * r.alpha;
        return r;
    }
    const double d = lambda > mu ? lambda - mu : mu - lambda, lo = lambda > mu ? mu : lambda;
    const double w = -expm1(-d * t), D = d + lo * w;
    r.alpha = mu * w / D;
    r.beta = lambda * w / D;
    const double below_one = 1.0 - 0x1p-53;
    if (!(r.alpha < 1.0)) r.alpha = below_one;
    if (!(r.beta < 1.0)) r.beta = below_one;
    r.coeff = 1 - r.alpha - r.beta;
    return r;
}
// Per transition matrix of the two-rate kernel: q = (1-alpha)(1-beta).  zero carries the reference's saturation rule
// (matrix_cache.cpp:153, probability.cpp:154) over to coeff = 1 - alpha - beta: a convention that keeps the model continuous
// at mu = lambda (the recurrence itself is well defined wherever alpha, beta < 1).  A 32-byte struct next to the 24-byte
// SlotParam: K1 and the per-family kernel are one body each, instantiated on the slot type (bd_matrix_build.h,
// family_lambda_kernel.h), and the lambda = mu instantiation loads and keeps live no second ratio.
struct SlotParamLM {
    static constexpr bool two_rates = true;
    double alpha;
    double beta;
    double q;
    int32_t zero;
    int32_t pad;
};
inline SlotParamLM slot_param_lm(long lq, long mq, long tq) {
    const BdRates r = bd_rates(double(lq) / 1000000000.0, double(mq) / 1000000000.0, double(tq) / 1000.0);
    SlotParamLM sp;
    sp.alpha = r.alpha;
    sp.beta = r.beta;
    sp.q = (1 - r.alpha) * (1 - r.beta);
    sp.zero = !(r.coeff > 0 && r.coeff != 1);
    sp.pad = 0;
    return sp;
}
// What the kernels that are one body for both slot types ask of a slot besides alpha and zero: the ratio of p1's geometric
// tail and q = (1-alpha)(1-tail)
__host__ __device__ inline double slot_tail(const SlotParam& sp) { return sp.alpha; }
__host__ __device__ inline double slot_q(const SlotParam& sp) { return sp.oma2; }
__host__ __device__ inline double slot_tail(const SlotParamLM& sp) { return sp.beta; }
__host__ __device__ inline double slot_q(const SlotParamLM& sp) { return sp.q; }
// A row-major pool of matrices of order n, not yet placed (base null, no extents)
inline MatrixPool row_major_pool(int n) {
    MatrixPool p{};
    p.n = n; p.ld = (n + 15) / 16 * 16; p.stride = (int64_t)n * p.ld; p.rows = n; p.k_valid = n; p.kmajor = 0;
    return p;
}

// Likelihood panels: [category][row][family], family fastest, so that a node's panel is the
// GEMM's B operand with the family axis as its N dimension.
//
// One K2 LAUNCH carries the GEMMs of a GROUP of mutually independent branches (the ready nodes of a tree level that share
// an epilogue variant): per branch one GemmOp in a device array, per launch one GemmArgs by value.  A workgroup's tile list
// (tile_plan_kernel) names, per tile, the op it belongs to; the kernel fetches that op's descriptor with scalar loads while
// the previous tile computes.  Small nodes fill the persistent grid together and a launch's tail overlaps the next node's
// head ("one launch (or one persistent-kernel phase) per height"; reference loop src/core.cpp:133-144).
struct GemmOp {
    int32_t slot[kMaxCategories];   // matrix of the child's branch per category (k-major pool)
    const double* src;              // child panel, rows = child sizes 0..M
    double* dst;                    // parent panel, or (dst_ldt > 0) the child's transposed factor panel
    int64_t src_kstride;            // doubles between the categories of src / dst / gath_src
    int64_t dst_kstride;
    int64_t gath_kstride;
    int32_t ld;                     // leading dimension of src and of a row-major dst = GEMM columns (multiple of kBN)
    int32_t rows;                   // GEMM rows = parent sizes 1..rows: M, or R when the parent is the root
    int32_t out_off;                // panel row of parent size 1: 1 (interior parent; row 0 is copied), 0 (root)
    int32_t n_row_tiles;            // ceil(rows / (16 * GemmArgs::mi)): filled per call
    int32_t n_col_tiles;
    // > 0: a factor GEMM, stored transposed: dst[column][16 - out_off + panel row], dst_ldt rows per column
    int32_t dst_ldt;
    // one leaf sibling folded into the epilogue (K3's work for a parent with one leaf and interior children)
    int32_t n_leaf;
    int32_t taxon;                  // row of `counts`
    int32_t leaf_slot[kMaxCategories];
    const int32_t* counts;          // [row][column] observed counts
    int64_t counts_ld;
    // factor panel of an interior sibling with fewer distinct columns than the parent, folded into the epilogue:
    // column f of the parent takes column gath_map[f] of the TRANSPOSED factor gath_src (gath_ld rows per column)
    const double* gath_src;
    int64_t gath_ld;
    const int32_t* gath_map;
    // per (category, column tile) of the CHILD panel: rows outside [bext[..][0], bext[..][1]] are exactly zero (extents.hip);
    // nullptr: unknown
    const int32_t* bext;
    // Joint K ranges (range_kernel, extents.hip; nullptr: no extents, every k-step): per (category, column tile, 16-row block
    // of the matrix) the first and last k-step (4 deep) this op's MFMAs need, lo | hi << 16, lo > hi: none --
    // jr[((category * jr_nct + (column tile & jr_ct_mask)) * (ext_blocks + kRangePad)) + block].  jr_nct = 1 and jr_ct_mask = 0
    // where the panels have no extents (the ranges are then the matrix's own).  The planner takes a tile's K tiles from the
    // hull of its blocks' ranges; K2 reads its MI ranges from here.
    const int32_t* jr;
    int32_t jr_nct, jr_ct_mask;
    // upper bounds of the child panel's magnitudes (node_level_kernel): [category][column tile][row steps], or nullptr
    const int32_t* bbound;
    // the child panel's narrowed hulls (ExtNode::narrow), laid out like bext: where range_kernel starts to look when it has
    // magnitude tables, and outside which it takes every bound as "all zero"; nullptr: none
    const int32_t* bnarrow;
};
constexpr int kRangePad = 8;        // blocks a row tile may overhang the matrix's last one (MI - 1): entries past it say "none"

struct GemmArgs {
    MatrixPool pool;                // k-major pool
    MatrixPool lpool;               // row-major pool (fused leaf siblings)
    const GemmOp* ops;              // the group's descriptors (device memory)
    int32_t n_ops;
    int32_t k_valid;                // contraction extent M+1
    int32_t kb;                     // depth of a K tile: 8, 12 or 16
    int32_t mi;                     // row tile = 16*mi, the same for every op of the launch
    int32_t n_categories;
    int32_t uniform_ld;             // > 0 (several column chunks, one column per family): columns of every panel in this chunk;
                                    // overrides GemmOp::ld / n_col_tiles
    int64_t f0;                     // first family of the chunk (offset into `counts`)
    const double* err;              // [(M+1)][3] error model of the fused leaf sibling, or nullptr
    int32_t max_family_size;
    unsigned long long* stamps;     // diagnostic: 6 words per workgroup (placement, epilogue ticks, tiles, lifetime), nullptr in production
    // Tile lists laid out by tile_plan_kernel (extents.hip): workgroup `local` of XCD `xcd` runs the tiles
    // plan[(xcd * blocks_per_xcd + local) * plan_rounds + i], i = 0, 1, ... until an entry with y == 0.
    // x: op << 24 | index of the tile in the op's list for that XCD (pair-major, row tile fastest),
    // y: first K tile << 16 | number of K tiles.
    const int2* plan;
    int32_t plan_rounds;
};
constexpr int kMaxGroupOps = 128;   // ops per K2 launch (7 bits of a plan entry)

// One K2 launch as the tile planner sees it.  K loops of unequal length (zero extents) make a fixed deal of tiles uneven:
// the planner deals each round of tiles (one per workgroup of the XCD, in the order the fixed deal would run them, so the
// row tiles of a column tile still run together) longest tile to least-loaded workgroup.  The XCD's list is the
// concatenation of the lists of the launch's ops.
struct PlanLaunch {
    const int32_t* aext;            // k-major pool extents (MatrixPool::ext), or nullptr: every K tile
    int32_t ext_blocks;
    const GemmOp* ops;              // slot[], bext, n_row_tiles, n_col_tiles of every op
    int32_t n_ops;
    int32_t uniform_ld;             // as GemmArgs
    int32_t mi, n_categories, k_valid;
    int32_t kb;                     // depth of a K tile (GemmArgs::kb)
    int32_t blocks_per_xcd;         // workgroups of the launch / 8
    int32_t rounds;                 // list length per workgroup
    int32_t fixed;                  // what an output tile costs beyond its K loop, in K tiles
    int32_t bias;                   // percent: the first-dispatched workgroup of a CU (local index < 32 of 64) runs that much faster
    int32_t bias3[4];               // three or four workgroups per CU (96 / 128 per XCD; local indices j, j + 32, ... share a CU): what a K
                                    // tile costs the first / second / ... dispatched one, in percent of the mean
    int2* plan;                     // [8][blocks_per_xcd][rounds]
};
constexpr int kPlanSlack = 2;       // spare list entries per workgroup (the planner's last rounds are dealt as one batch)
// max_rounds: the longest PlanLaunch::rounds of the launches (the planner's grid depth)
hipError_t launch_tile_plan(const PlanLaunch* d_launches, int n_launches, int max_rounds, hipStream_t stream);
// Workgroups of K2 resident on a CU.  Row tiles of up to 80 rows: four with 8- and 12-deep K tiles (26 / 39 KB of LDS each: four
// times 39 936 bytes, allocated in 1 280-byte granules, are exactly a CU's 160 KB; 128 vector registers), three with 16-deep ones (52 KB with an unpadded B tile, <= 168 registers); the taller ones: two (<= 250
// registers).
constexpr int prune_gemm_wg_per_cu(int mi, int kb) { return mi <= 5 ? (kb <= 12 ? 4 : 3) : 2; }
constexpr int kPlanLanes = 128;     // workgroups of an XCD the tile planner can deal to (32 CUs x 3 = 96 on MI355X)
// workgroups of a K2 launch (a multiple of 8) whose busiest XCD owns `tiles_xcd0` tiles: as many as are resident, fewer when there are fewer tiles
int prune_gemm_blocks(int64_t tiles_xcd0, int n_cu, int mi, int kb);
// tiles XCD 0 owns of an op with n_pairs = categories * column tiles
inline int64_t prune_gemm_tiles_xcd0(int n_categories, int n_col_tiles, int n_row_tiles) {
    return (((int64_t)n_categories * n_col_tiles + 7) / 8) * n_row_tiles;
}

struct GatherArgs {
    int32_t n_leaf;
    int32_t taxon[kMaxLeafPerOp];
    int32_t slot[kMaxLeafPerOp][kMaxCategories];
    const int32_t* counts;          // [taxon][family] for the whole shard
    int64_t counts_ld;
    double* dst;
    int64_t panel_kstride;          // doubles between the categories of dst
    int32_t ld;
    int32_t row_off;
    int32_t rows;
    int32_t rows_store;
    int32_t mode;
    // factor panels of interior children that have fewer distinct columns than this parent (subtree-level
    // de-duplication): column f of the parent takes column map[j][f] of factor j.  Factors are stored TRANSPOSED by
    // their GEMM (prune_gemm.hip, TRANS): src[j][category][column][15 + row_off + panel row], ld_src rows per column.
    int32_t n_src;
    const double* src[2];
    int64_t ld_src[2];
    int64_t kstride_src[2];         // doubles between the categories of src[j]
    const int32_t* map[2];
    // [category][ld / 128][2] zero extent of each 128-column tile of dst (extents.hip), or nullptr: rows outside it (rounded
    // out to K2's 16-row K tiles) are neither read nor written by the assemble pass
    const int32_t* tileext;
    // TRANSPOSED copies of the leaf children's row-major matrices (leaf_transpose_kernel), laid out like a factor:
    // lt[l][category][count x][15 + row s] = P_leaf[s][x], ld_src[0] doubles per count -- so that the assemble pass reads a
    // leaf's factor as whole lines, like the interior children's, instead of one 8-byte element per matrix row.  nullptr: none
    // (the pass then gathers from the row-major matrix on its way out).
    const double* lt[kMaxLeafPerOp];
    int64_t lt_kstride;             // doubles between the categories of lt[l]
};
// One transposed copy per (leaf branch that takes part in an assemble pass, category): src slot of the row-major pool -> dst.
struct LeafTArgs {
    MatrixPool pool;                // row-major pool
    const int32_t* pairs;           // [n_pairs] branch (pair index of the row-major pool); slot = category * pool_pairs + pair
    int32_t pool_pairs;
    int32_t n_list;                 // entries of `pairs`
    int32_t n_x;                    // counts 0..n_x-1 (columns of P read)
    int32_t ld_t;                   // doubles per count in dst
    double* dst;                    // [pair][category][n_x][ld_t]
    int64_t kstride;                // doubles between categories
    int64_t pair_stride;            // doubles between pairs
};
hipError_t launch_leaf_transpose(const LeafTArgs& a, int n_pairs, int n_categories, hipStream_t stream);

// Zero extents of the likelihood panels (extents.hip).  One ExtNode per interior non-root node, static per context.
constexpr int kMaxExtChildren = 4;
struct ExtNode {
    int32_t cols;                            // padded columns of the node's panel
    int32_t n_leaf, n_inner;
    int32_t leaf_pair[kMaxExtChildren];      // the leaf child's branch: pair index in the row-major pool
    int32_t leaf_row[kMaxExtChildren];       // the leaf child's row in `cnt`
    const int32_t* cnt;                      // [leaf children][columns] observed counts
    int64_t cnt_ld;
    int32_t inner_pair[kMaxExtChildren];     // the interior child's branch: pair index in the k-major pool
    int32_t inner_cols[kMaxExtChildren];
    const int32_t* inner_map[kMaxExtChildren];      // this node's column -> the child's column (nullptr: the same)
    const int32_t* inner_colext[kMaxExtChildren];   // the child's per-column extents [category][its columns][2]
    int32_t* colext;                         // [category][cols][2]: rows outside [lo, hi] of a column are exactly zero
    int32_t* tileext;                        // [category][cols / 128][2]: hull over a 128-column tile (K2's B operand)
    // magnitude bounds (node_level_kernel): [category][cols / 128][row steps] per 128-column tile and step of 4 panel rows,
    // an upper bound of log2 of every COMPUTED entry, in 1/256 (kMagNone: all exactly zero); the interior children's likewise
    int32_t* bound;
    const int32_t* inner_bound[kMaxExtChildren];
    // [category][cols / 128][2]: the tile's hull cut back from both ends over the row steps that the magnitude bounds prove to
    // hold computed zeros only (node_level_kernel).  Contiguous, inside tileext; equal to it without magnitude tables or
    // with ExtArgs::narrow off.  The assemble passes write these rows only, and no K range reaches outside them.
    int32_t* narrow;
    const int32_t* inner_narrow[kMaxExtChildren];
};
struct ExtArgs {
    const ExtNode* nodes;
    int32_t first, count;                    // the nodes of one level (independent of each other)
    const int32_t* leaf_ext;                 // row-major pool: per slot and column x, first / last row s with P[s][x] != 0
    int32_t leaf_ext_blocks, n_pairs_leaf;
    const int32_t* kext;                     // k-major pool: per slot and block of 16 parent sizes, first / last child size
    int32_t kext_blocks, n_pairs_inner;
    int32_t M;
    const double* err;                       // error model or nullptr
    int32_t n_dev;
    // magnitude tables of this call's matrices (MagArgs), nullptr: no bounds
    const int32_t* t4;
    const int32_t* lt;
    int32_t n_rsteps, n_ksteps;
    int32_t n_cu;                            // compute units of the device: sizes the tiles a workgroup owns
    int32_t level_tiles;                     // diagnostic (cafe_debug_level_tiles): column tiles per workgroup, 0 = chosen per level
    int32_t narrow;                          // cut the hulls back by the bounds (ExtNode::narrow); 0: CAFE_NO_NARROW, they stay structural
};
// one launch per tree level: the intervals of the level's nodes and, with magnitude tables, the bounds of their panels
// missing: the counts may hold CAFE_COUNT_MISSING (the kernel's MISSING instantiation: such a leaf narrows no interval and
// bounds its factor by the magnitude of 1.0)
hipError_t launch_node_level(const ExtArgs& a, int max_col_tiles, int n_categories, hipStream_t stream, bool missing = false);

// Magnitudes (extents.hip).  A product P[s][k] L[k][f] of two non-zero factors below half the smallest denormal moves no
// accumulator either: the tables below bound log2 of the matrix entries, node_level_kernel propagates bounds of the panels
// up the tree, and range_kernel cuts a block's K range to the k-steps where (matrix bound + panel bound) >= kSkipBelow.
// All bounds are upper bounds of log2 in units of 1/256, rounded up.
constexpr int32_t kMagUnit = 256;
constexpr int32_t kMagNone = -(1 << 28);             // every entry exactly zero (two of them still add without overflow)
constexpr int32_t kMagFloor = -1050 * kMagUnit;      // a panel bound inside the exact extent is never below this: a sum of up to
                                                     // 2048 products, each rounded up in the denormal range, stays under 2^-1063
constexpr int32_t kMagSlack = 16;                    // added per tree level: (1 + 2^-53)^n of the roundings, the denormal round-ups
constexpr int32_t kSkipBelow = -1100 * kMagUnit;     // 2^-1100 * 4 products of an MFMA < 2^-1075: rounds away against 0 or >= 2^-1074
// Narrowed hulls.  A row step whose bound BEFORE the floor lies below kSkipBelow holds computed zeros only: a factor whose
// log-sum is below it is a sum of products that all round to zero, in any order and any fusion (the argument of the k-step
// skip), and a product of factors bounded below it rounds to zero.  node_level_kernel cuts such row steps off both ends of a
// tile's hull into a second interval (ExtNode::narrow).  The bound table keeps its floor over the whole structural hull; its
// readers -- the level above, range_kernel -- take the bound of a row step outside the narrowed interval as "all zero".
constexpr int kMaxSteps = 512;                       // k-steps / row steps of the largest matrix order (2048 / 4)
struct MagArgs {
    MatrixPool kpool, lpool;
    int32_t n_kslots, n_lslots;      // slots of this call
    int32_t n_ksteps;                // ceil((M + 1) / 4): steps of 4 child sizes (K2's k-steps)
    int32_t n_rsteps;                // ceil(N / 4): steps of 4 parent sizes 4r .. 4r + 3 (panel rows)
    int32_t M;
    int32_t* a16;                    // [k-major slot][k-step][ext_blocks]: largest entry of (16 parent sizes of a block) x (4 child sizes)
    int32_t* t4;                     // [k-major slot][k-step][row step]: largest over the step's parent sizes of sum_c P[s][c], c in the k-step
    int32_t* lt;                     // [row-major slot][count x <= M][row step]: largest P[s][x] over the step's sizes
};
hipError_t launch_magnitude_tables(const MagArgs& a, hipStream_t stream);
struct RangeArgs {
    const GemmOp* ops;
    int32_t n_ops;
    const int32_t* aext;             // MatrixPool::ext of the k-major pool
    int32_t ext_blocks;
    const int32_t* a16;              // MagArgs::a16, or nullptr: exact-zero extents only
    int32_t n_ksteps, n_rsteps, k_valid;
};
hipError_t launch_joint_ranges(const RangeArgs& a, int max_col_tiles, int n_categories, hipStream_t stream);

struct ReduceArgs {
    const double* root;             // root panel [category][i][family]
    int64_t panel_kstride;
    int32_t ld;
    int32_t R;
    int32_t K;
    int32_t model;                  // 0 base, 1 gamma, 2 root maximum (p-value path)
    const double* prior;            // [R]  (double)float prior
    const double* log_prior;        // [R]  log((double)float prior), host libm
    const double* cat_probs;        // [K]
    int64_t f0;                     // first family of the chunk
    int64_t nf;                     // families of the chunk that are real (not padding)
    double* fam_out;                // [F] lnL_f (base) / log(lik_f) (gamma)
    double* fam_lik;                // [F] lik_f (gamma)
    double* cat_out;                // [F][K] (gamma)
    int32_t* failed;                // [F]
};

// K1, overloaded on the slot type: SlotParam (bd_matrix.hip) and SlotParamLM (bd_matrix_lm.hip) are the two instantiations
template <class Slot>
hipError_t launch_bd_matrix_build(const MatrixPool& pool, const Slot* d_slots, int n_slots, hipStream_t stream);
template <class Slot>
hipError_t launch_bd_matrix_build_both(const MatrixPool& pool, const MatrixPool& kpool, const Slot* d_slots, const Slot* d_kslots, int n_slots,
                                       int n_kslots, hipStream_t stream);
// The kernels that keep a row of the recurrence in registers (K1, the per-family kernel) exist per number E of columns a lane
// owns: the smallest E of the list with cols <= 64 E.  Calls f(std::integral_constant<int, E>) and returns its result;
// hipErrorInvalidValue past 64 * 32 = bd_matrix_max_order() columns.
template <int... Es, class F>
hipError_t for_lane_width(std::integer_sequence<int, Es...>, int cols, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    (void)(... || (cols <= 64 * Es ? (e = f(std::integral_constant<int, Es>{}), true) : false));
    return e;
}
template <class F>
hipError_t for_lane_width(int cols, F&& f) {
    return for_lane_width(std::integer_sequence<int, 2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32>{}, cols, f);
}
// One launch for a group of ops.  variant: what the epilogue of EVERY op of the group does (the host groups by it):
//   mode (0 store, 1 multiply), leaf (0 none, 1 one leaf sibling, 2 gathered sibling factor), trans (factor GEMM, transposed store).
// blocks: prune_gemm_blocks of the group; events: attached to the dispatch.
struct GemmVariant { int mode, leaf, trans; };
hipError_t launch_prune_gemm(const GemmArgs& a, GemmVariant v, int blocks, hipStream_t stream, hipEvent_t ev_start = nullptr,
                             hipEvent_t ev_stop = nullptr);
int prune_gemm_pick_mi(int64_t row_tile_pairs_by_mi[10], int n_cu, int kb);     // row-tile height (in 16-row blocks) from the group's tile counts per height
// what a K3 launch of a group of ops shares
struct GatherGroup {
    MatrixPool pool;                // row-major pool
    const GatherArgs* ops;          // device array
    int32_t n_ops;
    int32_t n_categories;
    int32_t max_family_size;        // M
    const double* err;              // [(M+1)][n_dev] error model of the call, or nullptr
    int32_t n_dev;
    int32_t uniform_ld;             // > 0 (several column chunks): columns of every panel in this chunk, overrides GatherArgs::ld
    int64_t f0;                     // first family of the chunk (offset into `counts`)
    int32_t leaf_t;                 // this call filled the transposed leaf matrices (GatherArgs::lt): no error model, copies made
};
// One launch for a group of K3 ops of one variant (same n_leaf, n_src, mode; the error model is the call's): d_ops device
// array, h_ops the same on the host (grid extents).  missing: the counts may hold CAFE_COUNT_MISSING -- the MISSING
// instantiations of the three kernels; the transposed leaf copies are not read then (the planner makes none)
hipError_t launch_leaf_gather_group(const GatherGroup& g, const GatherArgs* h_ops, hipStream_t stream, bool missing = false);
hipError_t launch_root_reduce(const ReduceArgs& a, hipStream_t stream);
// sum_f w_f * fam_out[f] and the number of failed families -> out[0], out[1] (and out_host[0..1] when not null: pinned host memory)
hipError_t launch_final_sum(const double* fam_out, const double* weights, const int32_t* failed, int64_t n,
                            double* scratch, int n_scratch, double* out, double* out_host, hipStream_t stream);
hipError_t launch_mfma_probe(double* d_out, int iters, int blocks, hipStream_t stream);
int bd_matrix_max_order();

}  // namespace cafe
