// Host side of the C ABI (include/cafe_mi355x.h): context, per-call enqueue (the schedule's planner: cafe_schedule.hip).
//
// What of the reference this replaces, per scorer call:
//   base_model::infer_family_likelihoods   src/base_model.cpp:53-112
//   gamma_model::infer_family_likelihoods  src/gamma_core.cpp:169-246 (+ can_infer :123)
//   matrix_cache / matrix_cache_key        src/matrix_cache.h:42-61, src/matrix_cache.cpp:99-171
//   inference_prune                        src/core.cpp:133-144
// The tree is flattened once into a schedule of leaf-gather and GEMM launches (post-order,
// Sethi-Ullman child order so that few likelihood panels are live), families are de-duplicated
// once (build_reference_list, base_model.cpp:27) and stay resident on the device; a call uploads
// only the scalars that prepare_calculation changes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "cafe_call.h"
#include "root_family.h"

using namespace cafe;

namespace cafe {

void set_err(cafe_ctx* c, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
}

bool lambdas_valid(const cafe_ctx* c, const double* lam) {
    if (c->single_lambda) return lam[0] > 0;                                   // lambda.h:58
    for (int i = 0; i < c->n_lambdas; ++i) if (lam[i] < 0) return false;       // lambda.cpp:59
    return true;
}

// ... and the death rates of the context, when it has any: no rate may be negative (one lambda: that lambda > 0 as above)
bool rates_valid(const cafe_ctx* c, const double* lam, const double* mus) {
    if (!lambdas_valid(c, lam)) return false;
    for (int i = 0; mus && i < c->n_lambdas; ++i) if (!(mus[i] >= 0)) return false;
    return true;
}
bool rates_valid(const cafe_ctx* c, const double* lam) { return rates_valid(c, lam, context_mus(c)); }

int set_death_rates_impl(cafe_ctx* c, const double* mus) {
    if (!mus) { c->mus.clear(); return CAFE_OK; }
    // (each buffer on its own pointer: a setter that failed half way allocates only what is still missing)
    const size_t nb = sizeof(SlotParamLM) * (size_t)std::max(1, c->max_slots + c->max_kslots);
    if (!c->h_slots_lm) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipHostMalloc(&c->h_slots_lm, nb, hipHostMallocDefault));
        std::memset(c->h_slots_lm, 0, nb);
    }
    if (!c->d_slots_lm) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipMalloc(&c->d_slots_lm, nb));
        HIP_TRY(c, hipMemset(c->d_slots_lm, 0, nb));
    }
    c->mus.assign(mus, mus + c->n_lambdas);
    return CAFE_OK;
}

// The pinned stage (and the other pinned mirrors) may be rewritten once the last call's uploads from it have landed
int wait_for_stage(cafe_ctx* c) {
    if (c->upload_pending) { HIP_TRY(c, hipEventSynchronize(c->ev_upload)); c->upload_pending = false; }
    return CAFE_OK;
}

// Slot parameters of a call into the pinned stage: slot = k * n_pairs[layout] + pair, built from the de-quantized key
// like matrix_cache.cpp:148-149 (lambda.h:39, :82-88 for lambda * multiplier).
// Every category brings its own rates: the K of a gamma call share one (lambdas, mus) and differ in the multiplier, the G * K of a
// batch (cafe_score_batch) are K per parameter vector.  The two-rate parameters are written whenever the context has death
// rates set (a category's mus then stand in for the context's).
void fill_slots(cafe_ctx* c, const CategoryRates* cats, int K) {
    SlotParam* h[2] = {reinterpret_cast<SlotParam*>(c->h_stage), reinterpret_cast<SlotParam*>(c->h_stage) + c->max_slots};
    for (int layout = 0; layout < 2; ++layout) {
        const int P = c->n_pairs[layout];
        for (int k = 0; k < K; ++k)
            for (int p = 0; p < P; ++p) {
                long lq, mq;
                quantized_rates(cats[k].lambdas, cats[k].mus, c->pair_lam[layout][p], cats[k].multiplier, &lq, &mq);
                h[layout][k * P + p] = slot_param(lq, c->pair_tq[layout][p]);
                // death rates set: the two-rate kernel's parameters, same slots (the multiplier scales both rates)
                if (!c->mus.empty()) c->h_slots_lm[(layout ? c->max_slots : 0) + k * P + p] = slot_param_lm(lq, mq, c->pair_tq[layout][p]);
            }
    }
    c->last.n_slots = K * c->n_pairs[0];
    c->last.n_kslots = K * c->n_pairs[1];
    c->stats.n_matrices = (int64_t)K * c->n_distinct_pairs;
}
// ... of one parameter vector under the context's own death rates
void fill_slots(cafe_ctx* c, const double* lambdas, const double* multipliers, int K) {
    std::vector<CategoryRates> cats(K);
    for (int k = 0; k < K; ++k) cats[k] = {lambdas, context_mus(c), multipliers ? multipliers[k] : 1.0};
    fill_slots(c, cats.data(), K);
}

// K1 of a call whose slot parameters fill_slots left in the pinned mirrors: the lambda = mu kernels, or with death rates set
// the two-rate instantiations behind an upload of their own parameters
int upload_lm_slots(cafe_ctx* c, hipStream_t s) {
    if (c->mus.empty()) return CAFE_OK;
    const size_t n = (size_t)(c->max_slots + c->max_kslots);         // (the buffers hold max(1, n): a context without slots uploads nothing)
    if (n) HIP_TRY(c, hipMemcpyAsync(c->d_slots_lm, c->h_slots_lm, sizeof(SlotParamLM) * n, hipMemcpyHostToDevice, s));
    return CAFE_OK;
}
int launch_call_matrices(cafe_ctx* c, hipStream_t s) {
    if (c->mus.empty()) HIP_TRY(c, launch_bd_matrix_build_both(c->pool, c->kpool, c->d_slots, c->d_slots + c->max_slots, c->last.n_slots, c->last.n_kslots, s));
    else HIP_TRY(c, launch_bd_matrix_build_both(c->pool, c->kpool, c->d_slots_lm, c->d_slots_lm + c->max_slots, c->last.n_slots, c->last.n_kslots, s));
    return CAFE_OK;
}

// For the callers outside the scorer path (begin_matrix_call, cafe_call.h): slot parameters uploaded on `s`, K1 launched.  Afterwards
// slot_of[node * Kmax + k] (static) names the matrix of every branch and category.
int prepare_matrices(cafe_ctx* c, const double* lambdas, const double* multipliers, int K, hipStream_t s) {
    if (const int rc = wait_for_stage(c)) return rc;
    fill_slots(c, lambdas, multipliers, K);
    const size_t nb = sizeof(SlotParam) * (size_t)(c->max_slots + c->max_kslots);
    HIP_TRY(c, hipMemcpyAsync(c->d_params, c->h_stage, nb, hipMemcpyHostToDevice, s));
    if (const int rc = upload_lm_slots(c, s)) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_upload, s));
    c->upload_pending = true;
    return launch_call_matrices(c, s);
}

namespace {

// Host-only rejections; true => the call's value is +inf without touching the device.  (The gamma model's own apply to the
// scorer's reduction, not to cafe_root_posterior's.)
// One parameter vector: lambdas, mus ([n_lambdas], or nullptr: none), and with gamma_rules the K multipliers and alpha.
bool rejected(const cafe_ctx* c, const double* lambdas, const double* mus, bool gamma_rules, const double* multipliers, int K, double alpha) {
    if (!rates_valid(c, lambdas, mus)) return true;                            // base_model.cpp:56 / gamma_core.cpp:125
    if (!gamma_rules) return false;
    if (alpha < 0) return true;                                                // gamma_core.cpp:128
    // gamma_core.cpp:131-139: longest branch x largest multiplier x largest lambda saturated?
    bool first = true;
    double longest = 0;
    for (int v = 0; v < c->n_nodes; ++v) {       // clade::get_branch_lengths: the set of t > 0, root included
        double t = c->blen[v];
        if (!(t > 0.0)) continue;
        if (first || t > longest) { longest = t; first = false; }
    }
    double lm = *std::max_element(multipliers, multipliers + K);
    double ll = *std::max_element(lambdas, lambdas + c->n_lambdas);
    double lambda = lm * ll;
    // matrix_cache.cpp:115; with death rates: coeff = 1 - alpha - beta of that branch under the largest of either rate
    const double mu = !mus ? lambda : lm * *std::max_element(mus, mus + c->n_lambdas);
    return bd_rates(lambda, mu, longest).coeff < 0;
}
bool rejected(const cafe_ctx* c, const cafe_params* pr, const CallMode& m) {
    return rejected(c, pr->lambdas, context_mus(c), m.reduction == CallMode::kGamma && m.tail != CallMode::kPosterior, pr->multipliers, m.K, pr->alpha);
}

// Row-tile height of one K2 launch (a group of ops) from the (previous call's) non-zero extents of its matrices: a tile runs
// only the K tiles inside the union of its 16-row blocks' extents, so a lower tile hugs the band of a short branch more
// closely (at config 4 the launches execute 69 % of all K tiles with 144-row tiles, 64 % with 80-row ones) but is a little
// less efficient per MFMA and fills the persistent grid in different rounds.  Costs in units of one K tile of one 16-row
// block; the efficiency factors are measured (forced tile heights): even heights stage a padded A tile.
int pick_tile_height(const cafe_ctx* c, const int32_t* ext, const Group& g, int K, int64_t chunk_cols) {
    static const double eff[10] = {0, 0, 0, 0, 1.12, 1.03, 1.30, 1.06, 1.05, 1.00};
    const int nb = c->kpool.ext_blocks;
    const int kBK = c->kb;
    const int n_k = (c->M + 1 + kBK - 1) / kBK;
    const double overhead = 2.0 * 16 / kBK;  // prologue + epilogue of a tile, in K tiles
    int best = 9;
    double best_cost = 1e300;
    for (int mi = 9; mi >= 4; --mi) {
        if (mi == 6) continue;
        const int slots = prune_gemm_wg_per_cu(mi, c->kb) * c->n_cu / 8 * 8;
        double work = 0, tiles = 0;          // sum over (op, category, row tile, column tile) of (K tiles + overhead) * height; tiles
        for (int oi : g.ops) {
            const Op& op = c->ops[oi];
            const int rows = op.to_root ? c->R : c->M;
            const int n_col_tiles = (int)(panel_cols(c, op.child, chunk_cols) / kBN);
            const int row_tiles = (rows + 16 * mi - 1) / (16 * mi);
            for (int k = 0; k < K; ++k) {
                const int32_t* e = ext + (size_t)c->slot_of[(size_t)op.child * c->Kmax + k] * nb * 2;
                for (int rt = 0; rt < row_tiles; ++rt) {
                    int lo = 0x7fffffff, hi = -1;
                    for (int b = rt * mi; b < rt * mi + mi && b < nb; ++b) { lo = std::min(lo, e[2 * b]); hi = std::max(hi, e[2 * b + 1]); }
                    int nkt = n_k;
                    if (hi >= lo) nkt = std::min(hi, c->M) / kBK - lo / kBK + 1; else nkt = 1;
                    work += (nkt + overhead) * mi * n_col_tiles;
                }
            }
            tiles += (double)row_tiles * K * n_col_tiles;
        }
        const double rounds = std::ceil(tiles / slots);
        const double cost = std::max(work / slots, rounds * (work / tiles)) * eff[mi];
        if (cost < best_cost * (1.0 - 1e-9)) { best_cost = cost; best = mi; }
    }
    return best;
}

// Host side of a call's launches for K categories and a chunk `cols` columns wide: the tile height of every K2 group (from
// the previous call's extents when there are any), the per-op row-tile counts, the planner's descriptors.  sync: upload now
// (before a graph capture); otherwise on `s`, and only what changed since the last call.
int prepare_descriptors(cafe_ctx* c, DescSet& ds, int K, int64_t cols, const std::vector<int32_t>* prev_ext, bool sync, hipStream_t s, bool* plan_needed) {
    const size_t n_ops = c->h_gemm_ops.size();
    if (!ds.d_gemm_ops) {
        HIP_TRY(c, hipMalloc(&ds.d_gemm_ops, sizeof(GemmOp) * n_ops));
        HIP_TRY(c, hipMalloc(&ds.d_plan_desc, sizeof(PlanLaunch) * std::max(1, c->n_gemm_groups)));
        HIP_TRY(c, hipMalloc(&ds.d_plan, sizeof(int2) * std::max<size_t>(1, c->plan_entries)));
    }
    ds.group_mi.assign(c->n_gemm_groups, 0);
    ds.group_blocks.assign(c->n_gemm_groups, 0);
    ds.group_rounds.assign(c->n_gemm_groups, 0);
    ds.group_plan_off.assign(c->n_gemm_groups, 0);
    std::vector<GemmOp> ops = c->h_gemm_ops;
    std::vector<PlanLaunch> plans(c->n_gemm_groups);
    size_t used = 0;
    int gi = 0;
    for (const Group& g : c->groups) {
        if (g.type != 1) continue;
        int mi = c->force_mi;                               // 0: picked per launch
        if (!mi && prev_ext) mi = pick_tile_height(c, prev_ext->data(), g, K, cols);
        if (!mi) {                                          // no extents (yet): whole rounds x height
            int64_t tiles_by_mi[10] = {0};
            for (int h = 2; h <= 9; ++h)
                for (int oi : g.ops) {
                    const Op& op = c->ops[oi];
                    const int64_t gc = panel_cols(c, op.child, cols);
                    tiles_by_mi[h] += (int64_t)(((op.to_root ? c->R : c->M) + 16 * h - 1) / (16 * h)) * (gc / kBN) * K;
                }
            mi = prune_gemm_pick_mi(tiles_by_mi, c->n_cu, c->kb);
        }
        int64_t tiles0 = 0;
        for (int oi : g.ops) {
            const Op& op = c->ops[oi];
            GemmOp& d = ops[op.desc];
            d.n_row_tiles = (d.rows + 16 * mi - 1) / (16 * mi);
            const int64_t gc = panel_cols(c, op.child, cols);
            tiles0 += prune_gemm_tiles_xcd0(K, (int)(gc / kBN), d.n_row_tiles);
        }
        const int blocks = prune_gemm_blocks(tiles0, c->n_cu, mi, c->kb), nlb = blocks / 8;
        const int rounds = (int)((tiles0 + nlb - 1) / nlb) + kPlanSlack;
        const size_t need = (size_t)8 * nlb * rounds;
        if (used + need > c->plan_entries) { set_err(c, "internal: tile lists do not fit (%zu + %zu > %zu)", used, need, c->plan_entries); return CAFE_ERR_STATE; }
        PlanLaunch& L = plans[gi];
        L = PlanLaunch{};
        L.aext = c->kpool.ext; L.ext_blocks = c->kpool.ext_blocks;
        L.ops = ds.d_gemm_ops + g.first_desc; L.n_ops = (int)g.ops.size();
        L.uniform_ld = c->subtree_dedup || c->grouped ? 0 : (int32_t)cols;
        L.mi = mi; L.n_categories = K; L.k_valid = c->M + 1; L.kb = c->kb;
        L.blocks_per_xcd = nlb; L.rounds = rounds; L.fixed = std::max(1, c->plan_fixed * 8 / c->kb); L.bias = c->plan_bias;
        for (int i = 0; i < 4; ++i) L.bias3[i] = nlb == 128 ? c->plan_bias4[i] : (i < 3 ? c->plan_bias3[i] : 100);
        L.plan = ds.d_plan + used;
        ds.group_mi[gi] = mi; ds.group_blocks[gi] = blocks; ds.group_rounds[gi] = rounds; ds.group_plan_off[gi] = used;
        used += need;
        ++gi;
    }
    const bool ops_same = ds.gemm_ops_sent.size() == n_ops && std::memcmp(ds.gemm_ops_sent.data(), ops.data(), sizeof(GemmOp) * n_ops) == 0;
    const bool plans_same = ds.plan_desc_sent.size() == plans.size() &&
                            (plans.empty() || std::memcmp(ds.plan_desc_sent.data(), plans.data(), sizeof(PlanLaunch) * plans.size()) == 0);
    auto upload = [&](void* dst, void* stage, const void* src, size_t bytes) {
        if (sync) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
        std::memcpy(stage, src, bytes);      // (the previous upload from this pinned stage was waited for: ev_upload)
        return hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, s);
    };
    if (!ops_same) { HIP_TRY(c, upload(ds.d_gemm_ops, c->h_gemm_stage, ops.data(), sizeof(GemmOp) * n_ops)); ds.gemm_ops_sent = ops; }
    if (!plans_same && !plans.empty()) { HIP_TRY(c, upload(ds.d_plan_desc, c->h_plan_desc, plans.data(), sizeof(PlanLaunch) * plans.size())); ds.plan_desc_sent = plans; }
    // with extents the lists follow this call's matrices: planned every call; without, only when something they depend on changed
    const bool static_ok = ds.plan_static_valid && ds.plan_static_K == K && ds.plan_static_cols == cols && ops_same && plans_same;
    *plan_needed = c->kpool.ext != nullptr || !static_ok;
    ds.plan_static_valid = true; ds.plan_static_K = K; ds.plan_static_cols = cols;
    return CAFE_OK;
}

// The extents the previous scorer call's matrices published, when it had the same K, for prepare_descriptors: copied into
// `ext`, since h_ext is this call's to overwrite.  nullptr: none.
const std::vector<int32_t>* previous_extents(const cafe_ctx* c, int K, std::vector<int32_t>& ext) {
    if (!(c->h_ext && c->h_ext_valid && c->h_ext_K == K)) return nullptr;
    ext.assign(c->h_ext, c->h_ext + (size_t)2 * K * c->n_pairs[1] * c->kpool.ext_blocks);      // (n_kslots of a call with K categories)
    return &ext;
}

// The five work counters of a call's K2 launches: record_call counts them from zero, a graph replay copies its capture's
void copy_work(cafe_stats& to, const cafe_stats& from) {
    to.gemm_flops = from.gemm_flops; to.gemm_bytes = from.gemm_bytes; to.gemm_flops_per_family = from.gemm_flops_per_family;
    to.gemm_flops_dense = from.gemm_flops_dense; to.gemm_launches = from.gemm_launches;
}
void reset_work(cafe_stats& st) { copy_work(st, cafe_stats{}); }

// The three parts of a call's device work (record_call below).  In front of the prune: NaN clearing, parameter upload, K1, the
// extent copy for the next call, magnitude tables, node levels, joint K ranges, leaf transposes.
int enqueue_prepass(cafe_ctx* c, const DescSet& ds, const CallMode& m, hipStream_t s, bool events) {
    const int K = m.K;
    const bool use_err = m.use_err;
    if (c->panels_dirty) {                   // the last call returned NaN: no stale NaN may meet a zero of a padded K step
        HIP_TRY(c, hipMemsetAsync(c->d_panels, 0, (size_t)c->stats.panel_bytes, s));
        c->panels_dirty = false;
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_params, c->h_stage, c->params_bytes, hipMemcpyHostToDevice, s));
    if (const int rc = upload_lm_slots(c, s)) return rc;
    if (events) HIP_TRY(c, hipEventRecord(c->ev[0], s));
    if (const int rc = launch_call_matrices(c, s)) return rc;
    if (events) HIP_TRY(c, hipEventRecord(c->ev[1], s));
    if (c->debug_fail_in > 0 && --c->debug_fail_in == 0) {                     // test hook: a device error in the middle of a call
        set_err(c, "injected failure (cafe_debug_fail_next)");
        return CAFE_ERR_DEVICE;
    }
    if (c->h_ext) {                          // this call's extents for the next one; lands while the K2 launches run
        HIP_TRY(c, hipMemcpyAsync(c->h_ext, c->kpool.ext, sizeof(int32_t) * 2 * (size_t)c->last.n_kslots * c->kpool.ext_blocks, hipMemcpyDeviceToHost, s));
        c->h_ext_valid = true;
        c->h_ext_K = K;
    }
    const bool mag = c->last.magskip = c->magskip && !use_err;   // (an error model's taps would need bounds of their own: exact extents then)
    if (mag) {                               // magnitude tables of this call's matrices: one pass over the two pools
        MagArgs ma{};
        ma.kpool = c->kpool; ma.lpool = c->pool;
        ma.n_kslots = c->last.n_kslots; ma.n_lslots = c->last.n_slots;
        ma.n_ksteps = c->n_ksteps; ma.n_rsteps = c->n_rsteps; ma.M = c->M;
        ma.a16 = c->d_mag_a16; ma.t4 = c->d_mag_t4; ma.lt = c->d_mag_lt;
        HIP_TRY(c, launch_magnitude_tables(ma, s));
    }
    if (c->panel_extents) {                  // zero extents of every node's panel for this call's matrices (extents.hip)
        ExtArgs ea{};
        ea.t4 = mag ? c->d_mag_t4 : nullptr; ea.lt = c->d_mag_lt; ea.n_rsteps = c->n_rsteps; ea.n_ksteps = c->n_ksteps;
        ea.nodes = c->d_ext_nodes;
        ea.n_cu = c->n_cu; ea.level_tiles = c->force_level_tiles; ea.narrow = mag && !c->no_narrow;
        ea.leaf_ext = c->pool.ext; ea.leaf_ext_blocks = c->pool.ext_blocks; ea.n_pairs_leaf = c->n_pairs[0];
        ea.kext = c->kpool.ext; ea.kext_blocks = c->kpool.ext_blocks; ea.n_pairs_inner = c->n_pairs[1];
        ea.M = c->M;
        ea.err = use_err ? c->d_err : nullptr; ea.n_dev = use_err ? c->n_dev : 0;
        for (const auto& L : c->ext_levels) {
            ea.first = L.first; ea.count = L.count;
            HIP_TRY(c, launch_node_level(ea, L.max_col_tiles, K, s, c->has_missing));
        }
    }
    if (c->d_jr) {                           // the K ranges of every K2 op, for the planner and for K2
        RangeArgs ra{};
        ra.ops = ds.d_gemm_ops; ra.n_ops = (int)c->h_gemm_ops.size();
        ra.aext = c->kpool.ext; ra.ext_blocks = c->kpool.ext_blocks;
        ra.a16 = mag ? c->d_mag_a16 : nullptr;
        ra.n_ksteps = c->n_ksteps; ra.n_rsteps = c->n_rsteps; ra.k_valid = c->M + 1;
        HIP_TRY(c, launch_joint_ranges(ra, std::max(1, c->jr_max_tiles), K, s));
    }

    if ((c->last.leaf_t = c->d_lt && !use_err)) {   // transposed copies of the leaf matrices that meet a factor in an assemble pass
        LeafTArgs lt{};
        lt.pool = c->pool; lt.pairs = c->d_lt_pairs; lt.pool_pairs = c->n_pairs[0]; lt.n_list = (int)c->lt_pairs.size();
        lt.n_x = c->M + 1; lt.ld_t = c->factor_ld; lt.dst = c->d_lt;
        lt.kstride = (int64_t)(c->M + 1) * c->factor_ld; lt.pair_stride = lt.kstride * c->Kmax;
        HIP_TRY(c, launch_leaf_transpose(lt, lt.n_list, K, s));
    }
    return CAFE_OK;
}

// The prune of one column chunk [f0, f0 + cols): the K3 / K2 launches of the schedule, in its order
int enqueue_chunk(cafe_ctx* c, const DescSet& ds, const CallMode& m, int64_t f0, int64_t cols, hipStream_t s, bool events) {
    const int K = m.K;
    const bool use_err = m.use_err, leaf_t = c->last.leaf_t;
    const int uniform_ld = (c->subtree_dedup || c->grouped) ? 0 : (int)cols;
    int gi = 0;
    for (size_t g_index = 0; g_index < c->groups.size(); ++g_index) {
        const Group& g = c->groups[g_index];
        if (g.type == 0) {
            GatherGroup gg{};
            gg.pool = c->pool;
            gg.ops = c->d_gather_ops + g.first_desc; gg.n_ops = (int)g.ops.size(); gg.n_categories = K;
            gg.max_family_size = c->M;
            gg.err = use_err ? c->d_err : nullptr; gg.n_dev = use_err ? c->n_dev : 0;
            gg.uniform_ld = uniform_ld;
            gg.f0 = c->subtree_dedup ? 0 : f0;
            gg.leaf_t = leaf_t ? 1 : 0;
            HIP_TRY(c, launch_leaf_gather_group(gg, c->h_gather_ops.data() + g.first_desc, s, c->has_missing));
            continue;
        }
        GemmArgs a{};
        a.pool = c->kpool; a.lpool = c->pool;
        a.ops = ds.d_gemm_ops + g.first_desc; a.n_ops = (int)g.ops.size();
        a.k_valid = c->M + 1; a.kb = c->kb; a.mi = ds.group_mi[gi]; a.n_categories = K;
        a.uniform_ld = uniform_ld;
        a.f0 = c->subtree_dedup ? 0 : f0;
        a.err = use_err ? c->d_err : nullptr; a.max_family_size = c->M;
        a.stamps = (c->stamps_launch < 0 || c->stamps_launch == (long)c->stats.gemm_launches) ? c->d_stamps : nullptr;
        a.plan = ds.d_plan + ds.group_plan_off[gi]; a.plan_rounds = ds.group_rounds[gi];
        if (events && c->gemm_ev_used + 2 <= c->gemm_ev.size()) {       // start / stop events ride on the dispatch itself
            HIP_TRY(c, launch_prune_gemm(a, g.variant, ds.group_blocks[gi], s, c->gemm_ev[c->gemm_ev_used], c->gemm_ev[c->gemm_ev_used + 1]));
            c->gemm_ev_used += 2;
        } else {
            HIP_TRY(c, launch_prune_gemm(a, g.variant, ds.group_blocks[gi], s));
        }
        c->stats.gemm_launches += 1;
        c->gemm_launches_info.push_back({(int)g_index, K, a.mi, cols});
        for (int oi : g.ops) {
            const Op& op = c->ops[oi];
            const double gc = (double)panel_cols(c, op.child, cols);
            const int rows = op.to_root ? c->R : c->M;
            c->stats.gemm_flops_dense += 2.0 * rows * (c->M + 1) * gc * K;
            c->stats.gemm_flops += 2.0 * rows * (c->M + 1) * gc * K;      // (cafe_executed_flops counts what the tiles really ran)
            c->stats.gemm_flops_per_family += 2.0 * rows * (c->M + 1) * (double)cols * K;
            c->stats.gemm_bytes += 8.0 * K * ((double)rows * (c->M + 1) + (double)(c->M + 1) * gc + (double)rows * gc);
        }
        ++gi;
    }
    return CAFE_OK;
}

// What stands behind a chunk's root panel: K4 under the call's root rule, or cafe_root_posterior's two kernels; behind the last
// chunk (d_out given) the final sum, unless the tail is the posterior's.  (The pair also goes straight into pinned host memory:
// cafe_score without a communicator reads it there after the stream has drained, no device-to-host copy.)
int enqueue_root_tail(cafe_ctx* c, const CallMode& m, int64_t f0, int64_t cols, double* d_out, hipStream_t s) {
    if (m.points > 0) {                      // a batch: one launch reduces every point's categories, one sums every point's families
        ReduceBatchArgs b{};
        b.root = c->d_panels + c->panels[c->root_panel].offset;
        b.panel_kstride = c->panels[c->root_panel].kstride; b.ld = (int32_t)cols; b.R = c->R; b.K = m.K / m.points; b.G = m.points;
        b.model = (int)m.reduction; b.root_sum = m.tail == CallMode::kSum;
        b.prior = c->d_prior; b.log_prior = c->d_logprior; b.cat_probs = c->d_catprobs;
        b.f0 = f0; b.nf = std::max<int64_t>(0, std::min<int64_t>(cols, c->F_uniq - f0)); b.F = c->F_uniq;
        b.fam_out = c->d_bfam_out; b.failed = c->d_bfailed;
        HIP_TRY(c, launch_root_reduce_batch(b, s));
        c->last.chunk_f0 = f0; c->last.chunk_nf = b.nf;
        if (d_out)
            HIP_TRY(c, launch_final_sum_batch(c->d_bfam_out, c->d_weights, c->d_bfailed, c->F_uniq, m.points, c->d_bscratch, c->n_scratch, d_out, c->h_bresult, s));
        return CAFE_OK;
    }
    ReduceArgs r{};
    r.root = c->d_panels + c->panels[c->root_panel].offset;
    r.panel_kstride = c->panels[c->root_panel].kstride; r.ld = (int)cols; r.R = c->R; r.K = m.K; r.model = (int)m.reduction;
    r.prior = c->d_prior; r.log_prior = c->d_logprior; r.cat_probs = c->d_catprobs;
    r.f0 = f0; r.nf = std::max<int64_t>(0, std::min<int64_t>(cols, c->F_uniq - f0));
    r.fam_out = c->d_fam_out; r.fam_lik = c->d_fam_lik; r.cat_out = c->d_cat_out; r.failed = c->d_failed;
    if (m.tail == CallMode::kPosterior) HIP_TRY(c, launch_root_posterior(r, *m.posterior, s));
    else if (m.tail == CallMode::kSum) HIP_TRY(c, launch_root_reduce_sum(r, s));
    else HIP_TRY(c, launch_root_reduce(r, s));
    c->last.chunk_f0 = f0; c->last.chunk_nf = r.nf;
    if (d_out && m.tail != CallMode::kPosterior)
        HIP_TRY(c, launch_final_sum(c->d_fam_out, c->d_weights, c->d_failed, c->F_uniq, c->d_scratch, c->n_scratch, d_out, c->h_result, s));
    return CAFE_OK;
}

// The device work of one call, enqueued on `s` (or recorded into a graph being captured on `s`): parameter upload,
// K1, the schedule (K2 / K3 launches), K4, the final sum into d_out.  Everything that changes between calls of the
// same shape travels through the parameter block; kernel arguments depend only on the CallMode.
int record_call(cafe_ctx* c, DescSet& ds, const CallMode& m, double* d_out, hipStream_t s, bool events, bool capturing) {
    reset_work(c->stats);
    c->last.desc = &ds;
    // ---- host: tile heights and descriptors (the previous call's extents are in h_ext: that call was waited for)
    std::vector<int32_t> prev_ext;
    const std::vector<int32_t>* prev = previous_extents(c, m.K, prev_ext);
    bool plan_needed = true;
    int64_t planned_cols = std::min<int64_t>(c->chunk_cols, c->Fp);
    if (!capturing) if (const int rc = prepare_descriptors(c, ds, m.K, planned_cols, prev, false, s, &plan_needed)) return rc;   // (a capture's: before it began)
    if (const int rc = enqueue_prepass(c, ds, m, s, events)) return rc;

    // ---- prune, chunk by chunk (one chunk unless the workspace is limited)
    c->gemm_ev_used = 0;
    c->gemm_launches_info.clear();
    for (int64_t f0 = 0; f0 < c->Fp; f0 += c->chunk_cols) {
        const int64_t cols = std::min<int64_t>(c->chunk_cols, c->Fp - f0);
        const bool last = f0 + c->chunk_cols >= c->Fp;
        if (cols != planned_cols) {          // the last chunk is narrower: its own descriptors and lists (same stream: in order)
            if (capturing) { set_err(c, "internal: a captured call cannot re-plan for a narrower last chunk"); return CAFE_ERR_STATE; }
            HIP_TRY(c, hipStreamSynchronize(s));             // the descriptors (and their pinned stage) are still in use by the chunks before
            if (const int rc = prepare_descriptors(c, ds, m.K, cols, prev, false, s, &plan_needed)) return rc;
            plan_needed = true;
            planned_cols = cols;
            ds.plan_static_valid = false;
        }
        // (several chunks with extents: the lists depend on this chunk's panel extents -- none: extents need one chunk -- and
        // on the matrices, the same for every chunk: no re-plan)
        if (plan_needed && c->n_gemm_groups > 0)
            HIP_TRY(c, launch_tile_plan(ds.d_plan_desc, c->n_gemm_groups, *std::max_element(ds.group_rounds.begin(), ds.group_rounds.end()), s));
        plan_needed = false;
        if (const int rc = enqueue_chunk(c, ds, m, f0, cols, s, events)) return rc;
        if (events && last) HIP_TRY(c, hipEventRecord(c->ev[2], s));
        if (const int rc = enqueue_root_tail(c, m, f0, cols, last ? d_out : nullptr, s)) return rc;
    }
    c->last.plan_launches = c->n_gemm_groups;
    if (events) { HIP_TRY(c, hipEventRecord(c->ev[3], s)); c->events_valid = true; }
    return CAFE_OK;
}

}  // namespace

int launch_call(cafe_ctx* c, const CallMode& m, double* d_out, hipStream_t s);

// rootmax: the p-value path (probability.cpp:273-317, 391-444) prunes with the plain lambda, no error model and
// no prior, and keeps max_j L_root[j] per family instead of the scorer's reduction.
int enqueue(cafe_ctx* c, const cafe_params* pr, double* d_out, hipStream_t s, bool rootmax, const RootPosteriorArgs* posterior) {
    c->last.had_comm = c->comm != nullptr;
    if (!pr || !pr->lambdas || (!rootmax && !pr->prior)) { set_err(c, "cafe_score: lambdas and prior are required"); return CAFE_ERR_ARGUMENT; }
    CallMode m;
    m.reduction = rootmax ? CallMode::kRootMax : pr->model == CAFE_MODEL_GAMMA ? CallMode::kGamma : CallMode::kBase;
    m.tail = posterior ? CallMode::kPosterior : !rootmax && c->root_rule == CAFE_ROOT_SUM ? CallMode::kSum : CallMode::kMax;
    m.posterior = posterior; m.use_err = !rootmax && c->n_dev > 0; m.two_rate = !c->mus.empty();
    const bool gamma = m.reduction == CallMode::kGamma;
    const int K = m.K = gamma ? pr->n_categories : 1;
    if (gamma && (K < 1 || K > c->Kmax || !pr->multipliers || !pr->cat_probs)) {
        set_err(c, "cafe_score: gamma model needs 1..%d categories with multipliers and cat_probs", c->Kmax);
        return CAFE_ERR_ARGUMENT;
    }
    if (!rootmax && (c->n_dev > 0) != (pr->error_model != nullptr)) {
        set_err(c, "cafe_score: error model %s but the problem was created with n_deviations=%d", pr->error_model ? "given" : "missing", c->n_dev);
        return CAFE_ERR_ARGUMENT;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = wait_for_stage(c)) return rc;
    open_call(c, K, s);
    c->events_valid = false;
    c->last.model = rootmax ? CAFE_MODEL_BASE : pr->model;

    if (rejected(c, pr, m)) {
        double* hr = reinterpret_cast<double*>(c->h_stage);
        hr[0] = 0.0; hr[1] = 1.0;
        HIP_TRY(c, hipMemcpyAsync(d_out, hr, 2 * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipEventRecord(c->ev_upload, s));
        c->upload_pending = true;
        c->stats.n_matrices = 0;
        reset_work(c->stats);
        c->last.state = LastCall::kRejected;
        return CAFE_OK;
    }

    // ---- the call's parameters into the pinned mirror of the device block
    fill_slots(c, pr->lambdas, gamma ? pr->multipliers : nullptr, K);
    double* h_prior = reinterpret_cast<double*>(c->h_stage + ((char*)c->d_prior - c->d_params));
    double* h_logprior = reinterpret_cast<double*>(c->h_stage + ((char*)c->d_logprior - c->d_params));
    double* h_cat = reinterpret_cast<double*>(c->h_stage + ((char*)c->d_catprobs - c->d_params));
    for (int j = 0; j < c->R; ++j) {
        const double eq = rootmax ? 1.0 : (double)pr->prior[j];    // compute() returns float (root_equilibrium_distribution.h:15)
        h_prior[j] = eq;
        h_logprior[j] = std::log(eq);
    }
    for (int k = 0; k < K; ++k) h_cat[k] = gamma ? pr->cat_probs[k] : 1.0;
    if (m.use_err) std::memcpy(c->h_stage + ((char*)c->d_err - c->d_params), pr->error_model, sizeof(double) * (size_t)(c->M + 1) * c->n_dev);

    if (const int rc = launch_call(c, m, d_out, s)) return rc;
    c->last.state = rootmax || posterior ? LastCall::kMatricesOnly : LastCall::kScored;
    return CAFE_OK;
}

// The device work of a call whose parameters stand in the pinned mirror: enqueued on `s`, or -- cafe_set_graphs -- captured once
// per graph key and replayed.  d_out: the pair of a single call, [points][2] of a batch.
int launch_call(cafe_ctx* c, const CallMode& m, double* d_out, hipStream_t s) {
    const int K = m.K;
    double* const own_out = m.points > 0 ? c->d_bresult : c->d_result;          // where a captured graph leaves its result
    const bool graph_ok = c->use_graph && !c->profile && !c->d_stamps && c->force_mi == 0 && c->force_level_tiles == 0 && m.tail != CallMode::kPosterior;
    if (!graph_ok) {
        if (const int rc = record_call(c, c->desc, m, d_out, s, c->profile != 0, false)) return rc;
    } else {
        const CallMode::GraphKey key = m.graph_key();
        cafe_ctx::CallGraph& cg = c->graphs[key];
        auto drop = [&]() { hipFree(cg.desc.d_gemm_ops); hipFree(cg.desc.d_plan_desc); hipFree(cg.desc.d_plan); c->graphs.erase(key); };
        if (!cg.exec) {
            // capture on the context's own stream (idle: calls are sequential), replay on the caller's.  The graph gets
            // descriptors and tile lists of its own, uploaded before the capture begins; its tile heights are frozen.
            if (c->stats.n_chunks > 1) { drop(); set_err(c, "cafe_set_graphs: a call in several column chunks cannot be captured"); return CAFE_ERR_STATE; }
            std::vector<int32_t> prev_ext;
            bool plan_needed = true;
            const int rp = prepare_descriptors(c, cg.desc, K, std::min<int64_t>(c->chunk_cols, c->Fp), previous_extents(c, K, prev_ext), true, c->stream, &plan_needed);
            if (rp != CAFE_OK) { drop(); return rp; }
            hipGraph_t graph = nullptr;
            HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            const int rc = record_call(c, cg.desc, m, own_out, c->stream, false, true);
            const hipError_t ee = hipStreamEndCapture(c->stream, &graph);
            if (rc != CAFE_OK) { if (graph) (void)hipGraphDestroy(graph); drop(); return rc; }
            if (ee != hipSuccess || !graph) { drop(); set_err(c, "hipStreamEndCapture failed: %s", hipGetErrorString(ee)); return CAFE_ERR_DEVICE; }
            const hipError_t ei = hipGraphInstantiate(&cg.exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ei != hipSuccess) { drop(); set_err(c, "hipGraphInstantiate failed: %s", hipGetErrorString(ei)); return CAFE_ERR_DEVICE; }
            cg.stats = c->stats;
        }
        copy_work(c->stats, cg.stats);
        c->last.chunk_f0 = (c->Fp - 1) / c->chunk_cols * c->chunk_cols;
        c->last.chunk_nf = std::max<int64_t>(0, std::min<int64_t>(c->chunk_cols, c->F_uniq - c->last.chunk_f0));
        HIP_TRY(c, hipGraphLaunch(cg.exec, s));
        if (d_out != own_out) HIP_TRY(c, hipMemcpyAsync(d_out, own_out, 2 * sizeof(double) * std::max(1, m.points), hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(c, hipEventRecord(c->ev_upload, s));
    c->upload_pending = true;
    return CAFE_OK;
}

// cafe_score_batch's buffers, sized for as many points as the context has categories (a batch cannot hold more); each on its
// own pointer: a call that failed half way allocates only what is still missing
static int ensure_batch_buffers(cafe_ctx* c) {
    const size_t G = (size_t)std::max(1, c->Kmax), F = (size_t)std::max<int64_t>(1, c->F_uniq), ns = (size_t)(2 * c->n_scratch + 1);
    if (!c->d_bfam_out) HIP_TRY(c, hipMalloc(&c->d_bfam_out, sizeof(double) * G * F));
    if (!c->d_bfailed) HIP_TRY(c, hipMalloc(&c->d_bfailed, sizeof(int32_t) * G * F));
    if (!c->d_bscratch) {
        HIP_TRY(c, hipMalloc(&c->d_bscratch, sizeof(double) * G * ns));
        const hipError_t e = hipMemset(c->d_bscratch, 0, sizeof(double) * G * ns);     // the tickets start at zero
        if (e != hipSuccess) { (void)hipFree(c->d_bscratch); c->d_bscratch = nullptr; HIP_TRY(c, e); }
    }
    if (!c->d_bresult) HIP_TRY(c, hipMalloc(&c->d_bresult, sizeof(double) * 2 * G));
    if (!c->h_bresult) HIP_TRY(c, hipHostMalloc(&c->h_bresult, sizeof(double) * 2 * G, hipHostMallocDefault));
    return CAFE_OK;
}

// cafe_score_batch up to its last launch.  live: the points the host did not reject, in batch order -- point live[i] rides as
// the categories i K .. i K + K - 1 of one call and leaves its pair in h_bresult[2 i ..]; a rejected point costs nothing.
int enqueue_batch(cafe_ctx* c, const cafe_batch_params* bp, std::vector<int>& live) {
    hipStream_t s = c->stream;
    c->last.had_comm = c->comm != nullptr;
    if (!bp || !bp->lambdas || !bp->prior) { set_err(c, "cafe_score_batch: lambdas and prior are required"); return CAFE_ERR_ARGUMENT; }
    if (bp->n_points < 1) { set_err(c, "cafe_score_batch: n_points must be at least 1"); return CAFE_ERR_ARGUMENT; }
    if (bp->model != CAFE_MODEL_BASE && bp->model != CAFE_MODEL_GAMMA) { set_err(c, "cafe_score_batch: unknown model %d", bp->model); return CAFE_ERR_ARGUMENT; }
    const bool gamma = bp->model == CAFE_MODEL_GAMMA;
    const int G = bp->n_points, K = gamma ? bp->n_categories : 1, L = c->n_lambdas;
    if (gamma && (K < 1 || !bp->multipliers || !bp->cat_probs || !bp->alpha)) {
        set_err(c, "cafe_score_batch: gamma model needs at least one category with multipliers, cat_probs and alpha of every point");
        return CAFE_ERR_ARGUMENT;
    }
    if ((int64_t)G * K > c->Kmax) {
        set_err(c, "cafe_score_batch: %d points x %d categories exceed the context's max_categories = %d", G, K, c->Kmax);
        return CAFE_ERR_ARGUMENT;
    }
    if ((c->n_dev > 0) != (bp->error_model != nullptr)) {
        set_err(c, "cafe_score_batch: error model %s but the problem was created with n_deviations=%d", bp->error_model ? "given" : "missing", c->n_dev);
        return CAFE_ERR_ARGUMENT;
    }
    if (c->comm) { set_err(c, "cafe_score_batch: not available on a context with a communicator attached"); return CAFE_ERR_STATE; }
    if (bp->mus && c->mus.empty()) { set_err(c, "cafe_score_batch: mus given but the context has no death rates set (cafe_set_death_rates)"); return CAFE_ERR_STATE; }

    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = wait_for_stage(c)) return rc;
    open_call(c, 0, s);
    c->events_valid = false;
    c->last.model = bp->model;
    auto mus_of = [&](int g) { return bp->mus ? bp->mus + (size_t)g * L : context_mus(c); };
    live.clear();
    for (int g = 0; g < G; ++g)
        if (!rejected(c, bp->lambdas + (size_t)g * L, mus_of(g), gamma, gamma ? bp->multipliers + (size_t)g * K : nullptr, K, gamma ? bp->alpha[g] : 0.0))
            live.push_back(g);
    const int Gl = (int)live.size();
    if (Gl == 0) {                           // nothing to build: every value is +inf
        c->stats.n_matrices = 0;
        reset_work(c->stats);
        c->last.state = LastCall::kBatch;
        return CAFE_OK;
    }
    if (const int rc = ensure_batch_buffers(c)) return rc;

    CallMode m;
    m.reduction = gamma ? CallMode::kGamma : CallMode::kBase;
    m.tail = c->root_rule == CAFE_ROOT_SUM ? CallMode::kSum : CallMode::kMax;
    m.use_err = c->n_dev > 0; m.two_rate = !c->mus.empty();
    m.points = Gl; m.K = Gl * K;
    c->last.K = m.K;

    // ---- the call's parameters into the pinned mirror of the device block
    std::vector<CategoryRates> cats((size_t)m.K);
    double* h_prior = reinterpret_cast<double*>(c->h_stage + ((char*)c->d_prior - c->d_params));
    double* h_logprior = reinterpret_cast<double*>(c->h_stage + ((char*)c->d_logprior - c->d_params));
    double* h_cat = reinterpret_cast<double*>(c->h_stage + ((char*)c->d_catprobs - c->d_params));
    for (int i = 0; i < Gl; ++i)
        for (int k = 0; k < K; ++k) {
            const int g = live[i];
            cats[(size_t)i * K + k] = {bp->lambdas + (size_t)g * L, mus_of(g), gamma ? bp->multipliers[(size_t)g * K + k] : 1.0};
            h_cat[(size_t)i * K + k] = gamma ? bp->cat_probs[(size_t)g * K + k] : 1.0;
        }
    fill_slots(c, cats.data(), m.K);
    for (int j = 0; j < c->R; ++j) {
        const double eq = (double)bp->prior[j];
        h_prior[j] = eq;
        h_logprior[j] = std::log(eq);
    }
    if (m.use_err) std::memcpy(c->h_stage + ((char*)c->d_err - c->d_params), bp->error_model, sizeof(double) * (size_t)(c->M + 1) * c->n_dev);

    if (const int rc = launch_call(c, m, c->d_bresult, s)) return rc;
    c->last.state = LastCall::kBatch;
    return CAFE_OK;
}

void collect_stats(cafe_ctx* c) {
    if (!c->events_valid) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->stats.ms_matrices = ms;
    if (hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) c->stats.ms_prune = ms;
    if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) c->stats.ms_reduce = ms;
    double g = 0;
    for (size_t i = 0; i + 1 < c->gemm_ev_used; i += 2)
        if (hipEventElapsedTime(&ms, c->gemm_ev[i], c->gemm_ev[i + 1]) == hipSuccess) g += ms;
    c->stats.ms_gemm = g;
}

int enqueue_rootmax(cafe_ctx* c, const double* lambdas, hipStream_t s) {
    cafe_params pr{};
    pr.model = CAFE_MODEL_BASE; pr.lambdas = lambdas; pr.n_categories = 1;
    return enqueue(c, &pr, c->d_result, s, true);
}

}  // namespace cafe

extern "C" {

double cafe_finish_partial(const double hp[2]) {
    if (std::isnan(hp[1])) return std::numeric_limits<double>::quiet_NaN();     // a shard failed its call (poisoned pair)
    if (hp[1] > 0) return std::numeric_limits<double>::infinity();
    return -hp[0];
}

int cafe_score_partial(cafe_ctx* ctx, const cafe_params* params, double* device_partial, void* hip_stream) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (!device_partial) { set_err(ctx, "cafe_score_partial: device_partial is NULL"); return CAFE_ERR_ARGUMENT; }
    const int rc = guarded(ctx, "cafe_score_partial", [&] { return enqueue(ctx, params, device_partial, (hipStream_t)hip_stream); });
    if (rc == CAFE_OK) return rc;
    // the caller owns the collective: a failed shard leaves rejects = NaN in its pair (best effort), so that a reduction over
    // the shards reads NaN on every rank (cafe_finish_partial returns NaN) even if this return code goes unread
    if (ctx->h_poison && ctx->device_ready) (void)hipMemcpyAsync(device_partial, ctx->h_poison, 2 * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)hip_stream);
    fail_after_enqueue(ctx, (hipStream_t)hip_stream);
    return rc;
}

// cafe_score behind a failed enqueue on a context with a communicator.  The call is collective: the other ranks are in the
// all-reduce or on their way into it, whatever went wrong here (a HIP error, an allocation, an exception -- argument errors are
// the same on every rank, but nothing relies on that).  Enter it with rejects = NaN: every rank then reads NaN and returns an
// error.  If even that cannot be enqueued, abort the communicator; the others run into their deadline (comm_wait_stream).
static void fail_together(cafe_ctx* ctx) {
    const std::string first = ctx->err;
    bool sent = hipSetDevice(ctx->device) == hipSuccess &&
                hipMemcpyAsync(ctx->d_result, ctx->h_poison, 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                comm_allreduce_pair(ctx, ctx->d_result, ctx->stream) == CAFE_OK;
    if (sent) sent = comm_wait_stream(ctx, ctx->stream) == CAFE_OK;
    if (!sent) comm_abort(ctx);
    set_err(ctx, "%s [rank %d of %d; the other ranks were %s]", first.c_str(), ctx->comm_rank, ctx->comm_world,
            sent ? "told through the all-reduce" : "NOT told: communicator aborted");
}

// cafe_score behind its enqueue: {sum lnL, rejects}, summed over the communicator's ranks when there is one, in h_result
static int read_score_pair(cafe_ctx* ctx) {
    if (const int rc = comm_allreduce_pair(ctx, ctx->d_result, ctx->stream)) { comm_abort(ctx); return rc; }   // family shards on other GPUs: one RCCL all-reduce
    // without a communicator K4's last kernel has already written the pair to h_result (a host-only rejection went
    // through a copy into d_result instead)
    if (ctx->comm || ctx->last.state == LastCall::kRejected)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_result, ctx->d_result, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = comm_wait_stream(ctx, ctx->stream)) return rc;
    ctx->upload_pending = false;
    if (ctx->comm && std::isnan(ctx->h_result[1])) {                    // (rejects is a sum of family weights: never NaN by itself)
        set_err(ctx, "cafe_score: another rank of the communicator failed its call (rank %d of %d read the poisoned pair)", ctx->comm_rank, ctx->comm_world);
        return CAFE_ERR_DEVICE;
    }
    return CAFE_OK;
}

int cafe_score(cafe_ctx* ctx, const cafe_params* params, double* neg_lnl, const cafe_family_out* out) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (!neg_lnl) { set_err(ctx, "cafe_score: neg_lnl is NULL"); return CAFE_ERR_ARGUMENT; }
    auto t0 = std::chrono::steady_clock::now();
    int rc = guarded(ctx, "cafe_score", [&] { return enqueue(ctx, params, ctx->d_result, ctx->stream); });
    if (rc == CAFE_OK) rc = read_score_pair(ctx);
    else if (ctx->comm) fail_together(ctx);
    if (rc != CAFE_OK) { fail_after_enqueue(ctx, ctx->stream); return rc; }
    *neg_lnl = cafe_finish_partial(ctx->h_result);
    if (std::isnan(ctx->h_result[0])) ctx->panels_dirty = true;        // NaNs may now sit in the panels (see record_call)
    ctx->stats.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    collect_stats(ctx);
    if (out) return cafe_family_results(ctx, out);
    return CAFE_OK;
}

int cafe_score_batch(cafe_ctx* ctx, const cafe_batch_params* params, double* neg_lnl) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (!neg_lnl) { set_err(ctx, "cafe_score_batch: neg_lnl is NULL"); return CAFE_ERR_ARGUMENT; }
    auto t0 = std::chrono::steady_clock::now();
    std::vector<int> live;
    int rc = guarded(ctx, "cafe_score_batch", [&] { return enqueue_batch(ctx, params, live); });
    // the batch's last kernel has written every live point's pair to h_bresult
    if (rc == CAFE_OK && !live.empty()) rc = comm_wait_stream(ctx, ctx->stream);
    if (rc != CAFE_OK) { fail_after_enqueue(ctx, ctx->stream); return rc; }
    ctx->upload_pending = false;
    for (int g = 0; g < params->n_points; ++g) neg_lnl[g] = std::numeric_limits<double>::infinity();
    for (size_t i = 0; i < live.size(); ++i) {
        const double* hp = ctx->h_bresult + 2 * i;
        neg_lnl[live[i]] = cafe_finish_partial(hp);
        if (std::isnan(hp[0])) ctx->panels_dirty = true;                // NaNs may now sit in the panels (see record_call)
    }
    ctx->stats.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    collect_stats(ctx);
    return CAFE_OK;
}

int cafe_family_results(cafe_ctx* ctx, const cafe_family_out* out) {
    if (!ctx || !out) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_family_results", kScorerResults)) return rc;
    if (const int rc = wait_last_call(ctx)) return rc;
    const int K = ctx->last.K;
    std::vector<double> tmp((size_t)ctx->F_uniq * std::max(1, K));
    std::vector<int32_t> itmp;
    if (out->family_lnl) {
        HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->d_fam_out, sizeof(double) * ctx->F_uniq, hipMemcpyDeviceToHost));
        spread_unique(ctx, tmp.data(), out->family_lnl);
    }
    if (ctx->last.model == CAFE_MODEL_GAMMA) {
        if (out->family_likelihood) {
            HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->d_fam_lik, sizeof(double) * ctx->F_uniq, hipMemcpyDeviceToHost));
            spread_unique(ctx, tmp.data(), out->family_likelihood);
        }
        if (out->category_likelihood) {
            HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->d_cat_out, sizeof(double) * ctx->F_uniq * K, hipMemcpyDeviceToHost));
            spread_unique(ctx, tmp.data(), out->category_likelihood, K);
        }
    }
    if (out->failed) {
        itmp.resize(ctx->F_uniq);
        HIP_TRY(ctx, hipMemcpy(itmp.data(), ctx->d_failed, sizeof(int32_t) * ctx->F_uniq, hipMemcpyDeviceToHost));
        spread_unique(ctx, itmp.data(), out->failed);
    }
    return CAFE_OK;
}

int cafe_root_max(cafe_ctx* ctx, const cafe_params* params, double* out) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (!out) { set_err(ctx, "cafe_root_max: out is NULL"); return CAFE_ERR_ARGUMENT; }
    int rc = guarded(ctx, "cafe_root_max", [&] { return enqueue(ctx, params, ctx->d_result, ctx->stream, true); });
    if (rc == CAFE_OK) rc = wait_last_call(ctx);
    if (rc != CAFE_OK) { fail_after_enqueue(ctx, ctx->stream); return rc; }
    ctx->upload_pending = false;
    collect_stats(ctx);
    if (ctx->last.state == LastCall::kRejected) {            // an invalid lambda has no matrices: the reference would throw (matrix_cache.cpp:90)
        set_err(ctx, "cafe_root_max: invalid lambda or death rate");
        return CAFE_ERR_ARGUMENT;
    }
    std::vector<double> tmp((size_t)ctx->F_uniq);
    HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->d_fam_out, sizeof(double) * ctx->F_uniq, hipMemcpyDeviceToHost));
    spread_unique(ctx, tmp.data(), out);
    return CAFE_OK;
}

int cafe_set_profiling(cafe_ctx* ctx, int on) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    ctx->profile = on ? 1 : 0;
    return CAFE_OK;
}

int cafe_set_death_rates(cafe_ctx* ctx, const double* mus) {
    return guarded(ctx, "cafe_set_death_rates", [&] { return set_death_rates_impl(ctx, mus); });
}

int cafe_set_root_rule(cafe_ctx* ctx, int32_t rule) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (rule != CAFE_ROOT_MAX && rule != CAFE_ROOT_SUM) { set_err(ctx, "cafe_set_root_rule: rule must be CAFE_ROOT_MAX or CAFE_ROOT_SUM"); return CAFE_ERR_ARGUMENT; }
    ctx->root_rule = rule;
    return CAFE_OK;
}

int cafe_get_root_rule(const cafe_ctx* ctx) { return ctx ? ctx->root_rule : CAFE_ROOT_MAX; }

int cafe_bd_rates(double lambda, double mu, double t, double out[3]) {
    if (!out) return CAFE_ERR_ARGUMENT;
    const SlotParamLM sp = slot_param_lm(quantize_lambda(lambda), quantize_lambda(mu), quantize_time(t));
    out[0] = sp.alpha; out[1] = sp.beta; out[2] = sp.zero;
    return CAFE_OK;
}

int cafe_set_graphs(cafe_ctx* ctx, int on) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    ctx->use_graph = on ? 1 : 0;
    return CAFE_OK;
}

int cafe_get_stats(const cafe_ctx* ctx, cafe_stats* stats) {
    if (!ctx || !stats) return CAFE_ERR_ARGUMENT;
    collect_stats(const_cast<cafe_ctx*>(ctx));
    *stats = ctx->stats;
    return CAFE_OK;
}

}  // extern "C"
