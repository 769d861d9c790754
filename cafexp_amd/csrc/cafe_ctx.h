// Internal: the context behind the C ABI handle and what the translation units of the library share.  cafe_create.hip builds
// it, cafe_score.hip is the scorer's call path, cafe_debug.hip reads it back; reconstruct.hip, marginal.hip, gradient.hip, history.hip,
// pvalues.hip and family_lambda.hip are the calls beside the scorer (their common frame: cafe_call.h), root_posterior.hip the one that
// runs the scorer's own path with other kernels behind the root panel, cafe_sharded.hip the multi-GPU layer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/cafe_mi355x.h"
#include "cafe_kernels.h"

namespace cafe {

struct Op {
    int type;                   // 0 assemble (leaf gathers and/or factor panels of de-duplicated children), 1 gemm
    int parent;                 // node whose panel is written (for a factor GEMM: the node the factor belongs to)
    bool to_factor;             // gemm: plain store of P_child . L_child over the CHILD's distinct columns
    int dst_panel;
    int src_panel;              // gemm
    int child;                  // gemm: child node (its branch's matrix)
    int n_leaf;                 // gather
    int leaf_node[kMaxLeafPerOp];
    int mode;                   // 0 store, 1 multiply
    int n_src;                  // assemble: factor panels folded in (children with fewer distinct columns than the parent)
    int src_child[2];
    int src_panels[2];
    bool to_root;
    // gemm: the factor panel of the parent's OTHER interior child (fewer distinct columns than the parent), folded into
    // this launch's epilogue through the parent->child column map
    bool has_gath;
    int gath_child;
    int gath_panel;
    int step;                   // ops of one step are mutually independent (see Group)
    int desc;                   // index of the op's descriptor in the context's GemmOp / GatherArgs array
    bool leaf_t = false;        // assemble: every leaf child has a transposed copy of its matrix (GatherArgs::lt)
};

// A likelihood panel (or the transposed factor panel of a de-duplicated child): where it lives in the arena d_panels
struct Panel {
    int64_t cols = 0;           // columns (multiple of kBN)
    bool factor = false;        // transposed factor: [category][column][factor_ld]; else [category][rows_pad][column]
    int64_t offset = 0;         // doubles from d_panels
    int64_t kstride = 0;        // doubles between categories
    int first_step = 0, last_step = 0;   // written first / read last in these steps (arena planning)
};

// One launch: the ops of one step that share a kernel variant.  Steps come from the dependency graph of the ops (an op
// reads the panels of its children and, when it multiplies, what an earlier op left in its own): all ops of a step are
// independent, so a step is a level of ready nodes (one launch per height; reference loop core.cpp:133-144).
struct Group {
    int type = 0;               // 1: K2 (prune_gemm), 0: K3 (leaf gather / assemble)
    int step = 0;
    std::vector<int> ops;       // indices into cafe_ctx::ops, descriptors contiguous from first_desc
    int first_desc = 0;
    GemmVariant variant{0, 0, 0};
    bool to_root = false;
};

// What a call's launches need beyond the static descriptors, per (reduction, K): tile heights, tile lists.  The context
// has one for the stream path (uploaded when it changes) and every captured graph one of its own.
struct DescSet {
    GemmOp* d_gemm_ops = nullptr;
    PlanLaunch* d_plan_desc = nullptr;
    int2* d_plan = nullptr;
    std::vector<GemmOp> gemm_ops_sent;
    std::vector<PlanLaunch> plan_desc_sent;
    std::vector<int> group_mi, group_blocks, group_rounds;     // per K2 group (index = position among the K2 groups)
    std::vector<size_t> group_plan_off;
    bool plan_static_valid = false;          // no extents: the lists depend on (K, tile heights, chunk width) only
    int plan_static_K = 0;
    int64_t plan_static_cols = 0;
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int64_t round_up64(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

struct RootPosteriorArgs;                    // root_sum.h

// The rates of one category of a call (fill_slots, cafe_score.hip): lambdas and mus are [n_lambdas], mus nullptr: mu = lambda
struct CategoryRates {
    const double* lambdas;
    const double* mus;
    double multiplier;
};

// What kind of scorer call this is, built once at the top of enqueue (cafe_score.hip): kernel arguments, the launches behind the
// root panel and the captured graph a call replays follow from it and from nothing else
struct CallMode {
    enum Reduction { kBase = 0, kGamma = 1, kRootMax = 2 } reduction = kBase;       // the values of ReduceArgs::model
    enum Tail { kMax, kSum, kPosterior } tail = kMax;    // K4 under either root rule, or cafe_root_posterior's two kernels on `posterior`
    const RootPosteriorArgs* posterior = nullptr;
    int K = 1;
    // cafe_score_batch: `points` parameter vectors of K / points categories each ride through the prune as the K categories of
    // this call; behind the root panel stand the batch's two kernels (root_reduce_batch.hip).  0: a single call.
    int points = 0;
    bool use_err = false, two_rate = false;  // error model; death rates set (K1's two-rate instantiation)
    struct GraphKey {                        // what a captured graph is captured for (cafe_ctx::graphs)
        int reduction, K; bool two_rate, root_sum; int points;
        bool operator<(const GraphKey& o) const {
            return std::tie(reduction, K, two_rate, root_sum, points) < std::tie(o.reduction, o.K, o.two_rate, o.root_sum, o.points);
        }
    };
    GraphKey graph_key() const { return {(int)reduction, K, two_rate, tail == kSum, points}; }
};

// What the last call left behind.  A call opens by setting state = kNone (open_call, cafe_call.h) and closes by setting its final
// state; the read-backs ask require_last.  The shape below the state is written as a call fixes it and stays until a later call
// writes it again: a call that builds matrices only leaves the launch shape of the scorer call before it in place.
struct LastCall {
    enum State {
        kNone,                               // nothing to read: fresh context, failed call, a matrix call not yet closed, cafe_score_per_family
        kRejected,                           // the host rejected the parameters (+inf): nothing was built
        kScored,                             // a scorer call: everything is readable
        kMatricesOnly,                       // root maximum, a closed posterior call, cafe_root_posterior: all but cafe_family_results
        kBatch                               // cafe_score_batch: the categories were several points' -- nothing a read-back could name
    } state = kNone;
    int K = 0, model = -1, n_slots = 0, n_kslots = 0;
    int64_t chunk_f0 = 0, chunk_nf = 0;      // the column chunk resident in the panels
    bool magskip = false, leaf_t = false, had_comm = false;   // magnitude tables / transposed leaf matrices used; a communicator attached as it began
    int plan_launches = 0;                   // K2 launches of the last recorded call
    const DescSet* desc = nullptr;           // its descriptors (diagnostics)
    hipStream_t stream = nullptr;            // the stream it was enqueued on
};

}  // namespace cafe

struct cafe_ctx {
    // problem
    int n_nodes = 0, n_taxa = 0, M = 0, R = 0, N = 0, n_lambdas = 1, single_lambda = 1, Kmax = 1, n_dev = 0, device = 0;
    int root = -1;
    std::vector<int> parent, lam_idx, leaf_taxon;
    std::vector<double> blen;
    std::vector<std::vector<int>> children;
    std::vector<std::vector<int>> inner, leaves;    // [n_nodes] interior / leaf children of a node, in child order
    int64_t F_all = 0, F_uniq = 0, Fp = 0;
    std::vector<int64_t> ref_of;            // family -> unique column
    std::vector<double> weights;
    // CAFE_FLAG_MISSING_COUNTS and at least one CAFE_COUNT_MISSING in the table: the schedule keeps leaves out of K2's epilogues
    // and off the transposed-leaf assemble, K3 and the extent pass run their MISSING instantiations (cafe_kernels.h:
    // count_is_missing), and the calls that have no such instantiation refuse the context (guarded_observed, cafe_call.h)
    bool has_missing = false;

    // schedule
    std::vector<cafe::Op> ops;
    std::vector<cafe::Panel> panels;         // by panel id (Op::dst_panel, ...)
    std::vector<cafe::Group> groups;         // launch order
    bool grouped = false;                    // one column chunk: every panel has its own place, steps hold many ops
    int n_gemm_ops = 0, n_gather_ops = 0, n_gemm_groups = 0;
    std::vector<cafe::GemmOp> h_gemm_ops;    // static part of the K2 descriptors (n_row_tiles is filled per call)
    std::vector<cafe::GatherArgs> h_gather_ops;
    cafe::GatherArgs* d_gather_ops = nullptr;
    // transposed copies of the row-major matrices of the leaf branches that meet an interior sibling's factor in an assemble
    // pass (GatherArgs::lt): [lt_pairs.size()][Kmax][M + 1][factor_ld], filled after K1 by every call without an error model
    double* d_lt = nullptr;
    int32_t* d_lt_pairs = nullptr;
    std::vector<int32_t> lt_pairs;           // pair index in the row-major pool
    cafe::GemmOp* h_gemm_stage = nullptr;    // pinned
    cafe::DescSet desc;                      // stream path
    bool panels_dirty = false;               // the last call returned NaN: stale NaNs may sit in padding rows; cleared before the next call
    // subtree-level de-duplication: a node's panel has one column per distinct pattern of leaf counts UNDER that node
    bool subtree_dedup = false;
    std::vector<int64_t> pat_cols;           // [n_nodes] padded distinct patterns of an interior node (0 for leaves)
    std::vector<char> edge_identity;         // [n_nodes] interior child whose columns are its parent's, in order
    std::vector<int32_t*> d_edge_map;        // [n_nodes] interior child: its column for every column of the parent
    std::vector<int32_t*> d_leaf_cnt;        // [n_nodes] interior parent: [its leaf children][its columns] observed counts
    std::vector<std::vector<int32_t>> h_edge_map, h_leaf_cnt;    // host copies (empty: none) until cafe_create uploads them
    std::vector<int> leaf_rank;              // [n_nodes] leaf: its row in the parent's d_leaf_cnt table
    int n_panels = 0, root_panel = -1;

    // device state
    bool device_ready = false;
    hipStream_t stream = nullptr;
    int32_t* d_counts = nullptr;
    double* d_weights = nullptr;
    cafe::MatrixPool pool{nullptr, 0, 0, 0, 0, 0, 0};     // row-major matrices of leaf branches (K3)
    cafe::MatrixPool kpool{nullptr, 0, 0, 0, 0, 0, 1};    // k-major matrices of interior branches (K2)
    // Matrix slots are static: one per (layout, distinct quantized branch length, lambda index) PAIR and category,
    // slot = category * n_pairs[layout] + pair, so the slots of a call with K categories are a prefix of the pool and
    // slot_of never changes.  (Two pairs whose lambda * multiplier happen to quantize alike are built twice.)
    int n_pairs[2] = {0, 0};                 // [0] leaf branches (row-major pool), [1] interior branches (k-major pool)
    std::vector<int> pair_of;                // [n_nodes] pair of the branch above a node (in its layout)
    std::vector<long> pair_tq[2];            // quantized branch length of a pair (matrix_cache.h:47)
    std::vector<int> pair_lam[2];            // lambda index of a pair
    int n_distinct_pairs = 0;                // distinct (t_q, lambda index) over both layouts: matrices the reference would build per category
    int max_slots = 0, max_kslots = 0;
    // per-call parameter block, one device allocation mirrored by the pinned h_stage (one upload per call):
    // [SlotParam x max_slots][SlotParam x max_kslots][prior R][log prior R][category probabilities Kmax][error model]
    char* d_params = nullptr;
    size_t params_bytes = 0;
    cafe::SlotParam* d_slots = nullptr;                   // [max_slots] row-major, then [max_kslots] k-major
    // cafe_set_death_rates: while `mus` is not empty every call builds its matrices with K1's two-rate
    // instantiation (bd_matrix_lm.hip) from slot parameters of their own -- device array and pinned mirror, [max_slots] row-major then
    // [max_kslots] k-major, allocated by the first call of the setter
    std::vector<double> mus;                 // [n_lambdas] death rate per lambda index; empty: lambda = mu
    cafe::SlotParamLM* d_slots_lm = nullptr;
    cafe::SlotParamLM* h_slots_lm = nullptr;
    // cafe_set_root_rule: what K4 (and the per-family root kernel) make of a root vector, CAFE_ROOT_MAX or CAFE_ROOT_SUM
    int root_rule = CAFE_ROOT_MAX;
    double* d_panels = nullptr;
    int64_t panel_stride = 0;               // doubles per panel
    int64_t panel_kstride = 0;              // doubles per category inside a panel
    int rows_pad = 0, kc = 0;
    int factor_ld = 0;                       // rows per column of a transposed factor panel
    int64_t chunk_cols = 0;
    size_t workspace_limit = 0;             // cafe_problem::workspace_limit (0 = automatic)
    double *d_prior = nullptr, *d_logprior = nullptr, *d_catprobs = nullptr, *d_err = nullptr;
    double *d_fam_out = nullptr, *d_fam_lik = nullptr, *d_cat_out = nullptr;
    int32_t* d_failed = nullptr;
    double* d_scratch = nullptr;
    int n_scratch = 1024;
    double* d_result = nullptr;
    // cafe_score_batch: per point (at most Kmax of them) a row of per-family values and flags, a scratch region with its ticket
    // for the final sum and a pair {sum lnL, rejects}, on the device and in pinned host memory; allocated by the first batch call
    double* d_bfam_out = nullptr;            // [Kmax][F_uniq]
    int32_t* d_bfailed = nullptr;            // [Kmax][F_uniq]
    double* d_bscratch = nullptr;            // [Kmax][2 * n_scratch + 1]
    double* d_bresult = nullptr;             // [Kmax][2]
    double* h_bresult = nullptr;             // pinned [Kmax][2]
    unsigned long long* d_stamps = nullptr;     // diagnostic block timeline of the LAST K2 launch (CAFE_GEMM_STAMPS=1)
    size_t stamps_words = 0;
    // pinned staging
    char* h_stage = nullptr;
    size_t stage_bytes = 0;
    double* h_result = nullptr;
    hipEvent_t ev_upload = nullptr;
    bool upload_pending = false;

    // multi-GPU: an RCCL communicator over the ranks that hold the other family shards (cafe_sharded.hip); with one
    // attached, cafe_score all-reduces {sum lnL, rejects} before the read-back
    void* comm = nullptr;                    // ncclComm_t
    bool comm_owned = false;
    int comm_world = 1, comm_rank = 0;
    // A call on a context with a communicator is collective.  A rank whose own enqueue fails still enters the all-reduce,
    // with rejects = NaN (h_poison), so that every rank returns an error instead of waiting for it; a rank that is gone
    // altogether is caught by the deadline below (the waiting ranks abort their communicator and return CAFE_ERR_DEVICE).
    double comm_timeout_s = 120.0;           // CAFE_COMM_TIMEOUT_S at cafe_comm_attach / cafe_create_sharded; <= 0: wait for ever
    double* h_poison = nullptr;              // pinned {0, NaN}
    // cafe_score_per_family (family_lambda.hip): its workspace, kept between calls and grown on demand
    void* pf_dev = nullptr;
    size_t pf_dev_bytes = 0;
    int64_t pf_max_batch = 0;                // CAFE_PER_FAMILY_BATCH: at most that many families per batch (diagnostic; 0 = what fits)
    double marginal_gemm_ms = 0, marginal_gemm_flops = 0;   // cafe_marginal_reconstruct: its GEMM launches (ms: while profiling)
    double change_band_ms = 0;                              // cafe_branch_change: its band kernel's launches (while profiling)
    double gram_ms = 0.0, gram_flops = 0.0;  // the Gram kernels of the last cafe_branch_scores (ms: profiling on)
    int history_batches = 0, history_passes = 0;            // cafe_sample_histories: column batches, draw passes per batch of the last call
    int debug_fail_in = 0;                  // cafe_debug_fail_next: the n-th next enqueue fails behind its K1 launch

    std::vector<int> slot_of;               // [node*Kmax + k]
    cafe::LastCall last;                    // what the last call left behind

    // launch
    int n_cu = 0;                            // compute units of the device (K2's persistent grid)
    long stamps_launch = -1;                 // CAFE_GEMM_STAMPS_LAUNCH, read once at cafe_create
    // A call's enqueue sequence is fixed per (reduction, K, rate model, root rule): upload, K1, the schedule, K4.  It can be captured
    // once in a hipGraph and replayed (one launch call instead of ~40 to ~300).  Off by default: on ROCm 7.2 the replay measured no
    // faster than the stream enqueue at the mammals size (base 0.47 vs 0.48 ms) and slower with K = 4 (0.62 vs 0.41 ms).
    struct CallGraph {
        hipGraphExec_t exec = nullptr;
        cafe_stats stats{};                  // the work counters of the captured sequence
        cafe::DescSet desc;                  // its own descriptors and tile lists (frozen at capture)
    };
    std::map<cafe::CallMode::GraphKey, CallGraph> graphs;
    int use_graph = 0;

    // zero extents of the likelihood panels (extents.hip): one descriptor per interior non-root node, grouped in levels of
    // mutually independent nodes (a node's level = 1 + its deepest interior child's); per node and category the per-column
    // and per-128-column-tile intervals outside which the panel is exactly zero
    bool panel_extents = false;
    bool no_asm_skip = false;                             // CAFE_NO_ASM_SKIP: the assemble pass writes every row (diagnostic)
    bool no_narrow = false;                               // CAFE_NO_NARROW: the magnitude bounds cut no row off the hulls (A/B runs, tests)
    std::vector<int32_t*> d_narrow;                       // [n_nodes] the narrowed hulls (ExtNode::narrow), beside d_tileext
    cafe::ExtNode* d_ext_nodes = nullptr;
    std::vector<int32_t*> d_colext, d_tileext;            // [n_nodes] (interior non-root nodes only)
    struct ExtLevel { int first, count, max_col_tiles; };
    std::vector<ExtLevel> ext_levels;
    // K steps whose products underflow (extents.hip, "Magnitudes"): the magnitude tables of a call's matrices, the bounds of
    // every planned node's panel, and -- whenever the matrices publish extents -- the joint K ranges of every K2 op
    bool magskip = false;                                 // panel_extents, no CAFE_NO_MAGSKIP, tables allocated
    int32_t *d_mag_a16 = nullptr, *d_mag_t4 = nullptr, *d_mag_lt = nullptr;
    std::vector<int32_t*> d_bound;                        // [n_nodes] (interior non-root nodes only)
    int32_t* d_jr = nullptr;                              // the ops' range tables, one allocation
    int n_ksteps = 0, n_rsteps = 0, jr_max_tiles = 0;

    // K2's row-tile height per launch is chosen from the non-zero extents of the PREVIOUS call's matrices (K1 publishes
    // them on the device; a copy lands in h_ext while the call's K2 launches run): the parameters of consecutive scorer
    // calls are close, and the choice only affects speed, never a bit of the result
    int32_t* h_ext = nullptr;                // pinned [max_kslots][ext_blocks][2]
    // tile lists of the K2 launches (tile_plan_kernel): one descriptor per launch, rebuilt per call (the tile heights may
    // change), uploaded when it differs from the last upload
    int plan_bias = 8;                       // percent by which the first-dispatched workgroup of a CU outruns the other (measured; CAFE_PLAN_BIAS)
    int plan_bias3[3] = {80, 100, 125};      // three workgroups per CU: cost of a K tile for the first / second / third dispatched (CAFE_PLAN_BIAS3=a,b,c)
    int plan_bias4[4] = {62, 88, 112, 160};  // four (CAFE_PLAN_BIAS4=a,b,c,d)
    int kb = 8;                              // depth of K2's K tiles: 8 or 12 (four workgroups per CU) or 16 (small matrices); CAFE_KB
    int plan_fixed = 8;                      // cost of an output tile beyond its K loop, in 8-deep K tiles (fitted: DESIGN.md; CAFE_PLAN_FIXED)
    size_t plan_entries = 0;
    cafe::PlanLaunch* h_plan_desc = nullptr;        // pinned
    bool h_ext_valid = false;
    int h_ext_K = 0;                         // categories of the call the copy belongs to

    // measurement
    struct GemmLaunch { int group; int K; int mi; int64_t cols; };   // what count_executed_flops needs (cols: the chunk's, several chunks only)
    std::vector<GemmLaunch> gemm_launches_info;
    int profile = 0;
    int force_level_tiles = 0;               // diagnostic: column tiles per workgroup of node_level_kernel (0 = chosen per level)
    int force_mi = 0;                        // diagnostic: K2 row-tile height for every launch (0 = chosen per launch)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> gemm_ev;
    size_t gemm_ev_used = 0;
    bool events_valid = false;
    cafe_stats stats{};

    std::string err;
};

namespace cafe {

void set_err(cafe_ctx* c, const char* fmt, ...);

#define HIP_TRY(c, expr)                                                                    \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            cafe::set_err(c, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return CAFE_ERR_DEVICE;                                                         \
        }                                                                                   \
    } while (0)

// A device allocation freed when it goes out of scope
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// Workspace of a call that cuts its work into batches: the caller's limit, else half of the free memory (counting the
// held_bytes of a workspace the caller keeps and will reuse), at most 8 GiB
inline hipError_t workspace_budget(size_t limit, size_t held_bytes, size_t* budget) {
    *budget = limit;
    if (limit) return hipSuccess;
    size_t free_b = 0, total_b = 0;
    const hipError_t e = hipMemGetInfo(&free_b, &total_b);
    *budget = std::min<size_t>((free_b + held_bytes) / 2, (size_t)8 << 30);
    return e;
}

// Columns of node v's panel (or of its factor) in a chunk `cols` wide: its distinct subtree patterns when the schedule
// de-duplicates subtrees, else the chunk's
inline int64_t panel_cols(bool dedup, const cafe_ctx* c, int v, int64_t cols) { return dedup ? c->pat_cols[v] : cols; }
inline int64_t panel_cols(const cafe_ctx* c, int v, int64_t cols) { return panel_cols(c->subtree_dedup, c, v, cols); }

// Host planner of cafe_create (cafe_schedule.hip): no HIP call, no environment; in the order cafe_create runs them
void plan_patterns(cafe_ctx* c, const cafe_problem* p, const std::vector<int64_t>& uniq, bool cherry_swap, double inherit_all, double inherit_big);
// commits the chosen schedule (ops, panels, chunk width, subtree_dedup, grouped); returns the arena's size in doubles
size_t plan_schedule(cafe_ctx* c, bool dedup, bool try_grouped, size_t budget, int64_t desc_cols);
std::vector<int> plan_extent_levels(cafe_ctx* c, bool matrix_extents);
size_t plan_leaf_transposes(cafe_ctx* c, double lt_min, size_t free_bytes, std::vector<int>& lt_of_pair);
void group_launches(cafe_ctx* c);
void dump_schedule(const cafe_ctx* c);

// cafe_create.hip
int create_impl(cafe_ctx* c, const cafe_problem* p);     // everything cafe_create does to a fresh context
void free_device(cafe_ctx* c);                            // releases what create_impl made, however far it got
// cafe_score.hip
bool lambdas_valid(const cafe_ctx* c, const double* lam);
bool rates_valid(const cafe_ctx* c, const double* lam);  // lambdas_valid, and no death rate of the context (cafe_set_death_rates) negative
bool rates_valid(const cafe_ctx* c, const double* lam, const double* mus);     // ... of `mus` ([n_lambdas], or nullptr: none)
int set_death_rates_impl(cafe_ctx* c, const double* mus);     // cafe_set_death_rates: [n_lambdas] or nullptr (lambda = mu again)
// the (lambda, mu) of lambda index i under multiplier `mult` as the matrix key quantizes them; mu = lambda without death rates
// (mus: [n_lambdas] death rates, nullptr: none)
inline void quantized_rates(const double* lambdas, const double* mus, int i, double mult, long* lq, long* mq) {
    *lq = quantize_lambda(lambdas[i] * mult);
    *mq = mus ? quantize_lambda(mus[i] * mult) : *lq;
}
inline const double* context_mus(const cafe_ctx* c) { return c->mus.empty() ? nullptr : c->mus.data(); }
// one scorer call enqueued on `s`, {sum lnL, rejects} -> d_out; rootmax: max_j L_root[j] per family instead (-> d_fam_out); posterior:
// cafe_root_posterior's two kernels where K4 and the final sum stand, on the stream path (no graph), without the gamma model's host rejection
int enqueue(cafe_ctx* c, const cafe_params* pr, double* d_out, hipStream_t s, bool rootmax = false, const RootPosteriorArgs* posterior = nullptr);
void collect_stats(cafe_ctx* c);                          // the profiling events of the last call into c->stats
// cafe_debug.hip: flops the K2 launches of the last call executed, from the extents it published (< 0: read-back failed)
double count_executed_flops(cafe_ctx* c, std::vector<double>* per_launch = nullptr, bool per_block = true, bool exact = false);
// One slot per distinct quantized (lambda * multiplier, t) and layout (matrix_cache.h:42-61), parameters uploaded on
// `s`, K1 launched: afterwards slot_of[node * Kmax + k] names the matrix of every branch and category.
int prepare_matrices(cafe_ctx* c, const double* lambdas, const double* multipliers, int K, hipStream_t s);
// Pupko reconstruction and Viterbi branch probabilities (reconstruct.hip)
int reconstruct_impl(cafe_ctx* c, const cafe_params* pr, const float* root_prior, int32_t* states);
int branch_probabilities_impl(cafe_ctx* c, const cafe_params* pr, const int32_t* sizes, double* out);
// Marginal reconstruction: posterior sizes, intervals and branch change probabilities (marginal.hip)
int marginal_impl(cafe_ctx* c, const cafe_params* pr, double level, const cafe_marginal_out* out);
// Per-family derivatives of log Z in the rates on the same two passes (gradient.hip: gradient_walk, sum_product.h); the same
// kept per branch, with their weighted Gram matrix (branch_scores.hip)
int branch_scores_impl(cafe_ctx* c, const cafe_params* pr, int32_t root_rule, const cafe_branch_scores_out* out);
void bd_rates_grad(double lambda, double mu, double t, double out[4]);     // plain doubles in, no quantization
// Ancestral histories drawn from the posterior of the same model (history.hip)
int history_impl(cafe_ctx* c, const cafe_params* pr, int32_t n_draws, uint64_t seed, const cafe_history_out* out);
// Device-side p-values (pvalues.hip) and what it needs from cafe_create.hip and cafe_score.hip: a context over the same tree
// whose family counts are written on the device, and the root-maximum prune of a context's families (-> d_fam_out, on stream s)
constexpr int32_t kFlagDeviceCounts = 0x40000000;        // internal cafe_problem flag
// (capture: cafe_debug_pvalues_stages' record of what the stages left, nullptr for cafe_pvalues -- no copy, no extra wait)
int pvalues_impl(cafe_ctx* c, const cafe_params* pr, int32_t n_simulations, uint64_t seed, double* pvalues, const cafe_pvalue_stages* capture = nullptr);
cafe_ctx* create_child_for_device_counts(const cafe_ctx* parent, int64_t n_families);
void destroy_child(cafe_ctx* c);
int enqueue_rootmax(cafe_ctx* c, const double* lambdas, hipStream_t s);
// one scorer evaluation per listed family, each under its own lambdas (family_lambda.hip)
int score_per_family_impl(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, double* family_lnl);
// ... each under its own (lambdas, mus): the same frame with the kernel's two-rate instantiation (family_lambda_lm.hip)
int score_per_family_lm_impl(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                             double* family_lnl);
// the root posterior of every family on the scorer's own prune (root_posterior.hip)
int root_posterior_impl(cafe_ctx* c, const cafe_params* pr, const cafe_root_posterior_out* out);
// multi-GPU (cafe_sharded.hip)
int comm_allreduce_pair(cafe_ctx* c, double* d_pair, hipStream_t s);
void comm_release(cafe_ctx* c);
// waits for `s`; with a communicator attached: under the deadline comm_timeout_s and watching the communicator's
// asynchronous error state -- on either the communicator is aborted and CAFE_ERR_DEVICE returned
int comm_wait_stream(cafe_ctx* c, hipStream_t s);
void comm_abort(cafe_ctx* c);

}  // namespace cafe
