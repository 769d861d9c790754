// cafe_create: the problem onto the device.  Range checks and family de-duplication, the matrix pools, the resident
// buffers, the schedule (the host planner: cafe_schedule.hip), the likelihood panels and the static launch descriptors.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "cafe_call.h"

using namespace cafe;

namespace cafe {

void free_device(cafe_ctx* c) {
    if (!c->device_ready) return;            // nothing was created on a device (argument / device errors)
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    comm_release(c);
    for (auto& g : c->graphs) if (g.second.exec) hipGraphExecDestroy(g.second.exec);
    hipFree(c->d_counts); hipFree(c->d_weights); hipFree(c->pool.base); hipFree(c->kpool.base); hipFree(c->kpool.ext); hipFree(c->pool.ext); hipFree(c->d_params); hipFree(c->d_panels);
    hipFree(c->d_ext_nodes); hipFree(c->d_mag_a16); hipFree(c->d_mag_t4); hipFree(c->d_mag_lt); hipFree(c->d_jr); hipFree(c->d_fam_out); hipFree(c->d_fam_lik); hipFree(c->d_cat_out); hipFree(c->d_failed);
    for (auto* ptrs : {&c->d_colext, &c->d_tileext, &c->d_narrow, &c->d_bound, &c->d_edge_map, &c->d_leaf_cnt}) for (auto ptr : *ptrs) hipFree(ptr);
    hipFree(c->d_scratch); hipFree(c->d_result); hipFree(c->d_stamps);
    for (void* h : {(void*)c->h_stage, (void*)c->h_result, (void*)c->h_ext, (void*)c->h_gemm_stage, (void*)c->h_plan_desc}) if (h) hipHostFree(h);
    auto free_desc = [](DescSet& d) { hipFree(d.d_gemm_ops); hipFree(d.d_plan_desc); hipFree(d.d_plan); d = DescSet(); };
    free_desc(c->desc);
    for (auto& g : c->graphs) free_desc(g.second.desc);
    hipFree(c->d_slots_lm); if (c->h_slots_lm) hipHostFree(c->h_slots_lm);
    hipFree(c->d_bfam_out); hipFree(c->d_bfailed); hipFree(c->d_bscratch); hipFree(c->d_bresult); if (c->h_bresult) hipHostFree(c->h_bresult);
    hipFree(c->d_gather_ops); hipFree(c->d_lt); hipFree(c->d_lt_pairs); hipFree(c->pf_dev);
    if (c->ev_upload) hipEventDestroy(c->ev_upload);
    for (auto& e : c->ev) if (e) hipEventDestroy(e);
    for (auto& e : c->gemm_ev) hipEventDestroy(e);
    c->graphs.clear();
    if (c->stream) hipStreamDestroy(c->stream);
}

namespace {

// Environment switches read at cafe_create, all diagnostics: none of them changes a result bit.  Those of the call path go
// into the context; those of cafe_create itself come back.
struct Switches { bool no_groups, no_kskip, no_magskip, no_leaf_t, no_cherry_swap, gemm_stamps, dump_schedule; double lt_min, inherit_all, inherit_big; int kb; };

Switches read_switches(cafe_ctx* c) {
    Switches sw{};
    const char* e;
    sw.no_groups = std::getenv("CAFE_NO_GROUPS");            // one op per launch from the slot pool instead of level-batched launches
    sw.no_kskip = std::getenv("CAFE_NO_KSKIP");              // no matrix or panel extents: every K tile of every launch
    sw.no_magskip = std::getenv("CAFE_NO_MAGSKIP");          // K ranges from the exact-zero extents alone, no magnitude bounds
    sw.no_leaf_t = std::getenv("CAFE_NO_LEAF_T");            // no transposed leaf matrices for the assemble passes
    sw.no_cherry_swap = std::getenv("CAFE_NO_CHERRY_SWAP");  // a cherry on one matrix keeps counts (a, b) and (b, a) in columns of their own
    sw.lt_min = (e = std::getenv("CAFE_LEAF_T_MIN")) ? atof(e) : 6.0;   // a leaf branch gets one when its passes write >= lt_min N columns
    // column-space thresholds of the subtree de-duplication (plan_patterns, step 2): "all,big"
    sw.inherit_all = 0.15; sw.inherit_big = 0.12;
    double th[2];
    if ((e = std::getenv("CAFE_INHERIT")) && std::sscanf(e, "%lf,%lf", &th[0], &th[1]) == 2 && th[0] >= 0 && th[1] >= 0) { sw.inherit_all = th[0]; sw.inherit_big = th[1]; }
    sw.kb = (e = std::getenv("CAFE_KB")) ? (std::atoi(e) == 16 ? 16 : std::atoi(e) == 12 ? 12 : 8) : 0;   // depth of K2's K tiles: 8, 12 or 16
    sw.gemm_stamps = std::getenv("CAFE_GEMM_STAMPS");        // per-workgroup block timeline of a K2 launch (cafe_debug_stamps)
    sw.dump_schedule = std::getenv("CAFE_DUMP_SCHEDULE");    // the launch list with its column counts, on stderr
    if ((e = std::getenv("CAFE_GEMM_STAMPS_LAUNCH"))) c->stamps_launch = std::atol(e);   // stamps of that K2 launch only
    if ((e = std::getenv("CAFE_PER_FAMILY_BATCH"))) c->pf_max_batch = std::max(0L, std::atol(e));   // cafe_score_per_family: families per batch
    c->no_asm_skip = std::getenv("CAFE_NO_ASM_SKIP") != nullptr;   // the assemble passes write every row
    c->no_narrow = std::getenv("CAFE_NO_NARROW") != nullptr;       // the hulls stay structural: the magnitude bounds cut no row off them
    if ((e = std::getenv("CAFE_FORCE_TILE")) && std::atoi(e) >= 2 && std::atoi(e) <= 9) c->force_mi = std::atoi(e);   // like cafe_debug_force_tile
    if ((e = std::getenv("CAFE_PLAN_FIXED"))) c->plan_fixed = std::max(0, atoi(e));   // the tile planner's cost of a tile beyond its K loop
    if ((e = std::getenv("CAFE_PLAN_BIAS"))) c->plan_bias = std::min(50, std::max(0, atoi(e)));   // first-dispatched workgroup of a CU, percent
    int v[4];                                                // a K tile's cost to the 1st .. 4th / 1st .. 3rd dispatched workgroup of a CU, percent
    if ((e = std::getenv("CAFE_PLAN_BIAS4")) && std::sscanf(e, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) == 4 && v[0] > 0 && v[1] > 0 && v[2] > 0 && v[3] > 0)
        std::copy(v, v + 4, c->plan_bias4);
    if ((e = std::getenv("CAFE_PLAN_BIAS3")) && std::sscanf(e, "%d,%d,%d", &v[0], &v[1], &v[2]) == 3 && v[0] > 0 && v[1] > 0 && v[2] > 0)
        std::copy(v, v + 3, c->plan_bias3);
    return sw;
}

// The tree and the family table: range checks, every node's interior and leaf children, family de-duplication
// (build_reference_list, base_model.cpp:27-51) and the column order.  uniq: the first family of every column.
int load_problem(cafe_ctx* c, const cafe_problem* p, std::vector<int64_t>& uniq) {
    const bool device_counts = p && (p->flags & kFlagDeviceCounts);      // internal: the caller fills d_counts on the device
    if (!p || p->n_nodes < 3 || !p->parent || !p->branch_length || !p->leaf_taxon || (!p->counts && !device_counts)) { set_err(c, "cafe_create: missing tree or family arrays"); return CAFE_ERR_ARGUMENT; }
    if (p->n_families < 1 || p->n_taxa < 2 || p->max_family_size < 1 || p->max_root_family_size < 1) { set_err(c, "cafe_create: empty family table or non-positive max sizes"); return CAFE_ERR_ARGUMENT; }
    c->n_nodes = p->n_nodes; c->n_taxa = p->n_taxa; c->M = p->max_family_size; c->R = p->max_root_family_size;
    c->N = std::max(c->M, c->R) + 1;                                   // base_model.cpp:77
    c->n_lambdas = std::max(1, p->n_lambdas); c->single_lambda = p->single_lambda;
    c->Kmax = std::max(1, p->max_categories); c->n_dev = p->n_deviations; c->device = p->device;
    if (c->Kmax > CAFE_MAX_CATEGORIES) { set_err(c, "cafe_create: more than %d gamma categories", CAFE_MAX_CATEGORIES); return CAFE_ERR_ARGUMENT; }
    c->parent.assign(p->parent, p->parent + p->n_nodes);
    c->blen.assign(p->branch_length, p->branch_length + p->n_nodes);
    c->leaf_taxon.assign(p->leaf_taxon, p->leaf_taxon + p->n_nodes);
    if (p->lambda_index) c->lam_idx.assign(p->lambda_index, p->lambda_index + p->n_nodes);
    else c->lam_idx.assign(p->n_nodes, 0);
    c->children.assign(p->n_nodes, {}); c->inner.assign(p->n_nodes, {}); c->leaves.assign(p->n_nodes, {});
    for (int v = 0; v < p->n_nodes; ++v) {
        int par = c->parent[v];
        if (par < 0) {
            if (c->root >= 0) { set_err(c, "cafe_create: more than one root"); return CAFE_ERR_ARGUMENT; }
            c->root = v;
        } else if (par >= p->n_nodes || par <= v) {
            set_err(c, "cafe_create: node %d: parent %d must come after its children", v, par); return CAFE_ERR_ARGUMENT;
        } else {
            c->children[par].push_back(v);
            (c->leaf_taxon[v] < 0 ? c->inner[par] : c->leaves[par]).push_back(v);
        }
        if (c->lam_idx[v] < 0 || c->lam_idx[v] >= c->n_lambdas) { set_err(c, "cafe_create: lambda index out of range at node %d", v); return CAFE_ERR_ARGUMENT; }
    }
    if (c->root < 0) { set_err(c, "cafe_create: no root"); return CAFE_ERR_ARGUMENT; }
    for (int v = 0; v < p->n_nodes; ++v) {
        bool leaf = c->children[v].empty();
        if (leaf != (c->leaf_taxon[v] >= 0) || (leaf && c->leaf_taxon[v] >= c->n_taxa)) { set_err(c, "cafe_create: leaf_taxon inconsistent with the tree at node %d", v); return CAFE_ERR_ARGUMENT; }
    }
    if (c->children[c->root].empty()) { set_err(c, "cafe_create: the root is a leaf"); return CAFE_ERR_ARGUMENT; }
    if (c->N > bd_matrix_max_order()) { set_err(c, "cafe_create: matrix order %d exceeds %d", c->N, bd_matrix_max_order()); return CAFE_ERR_ARGUMENT; }

    // families: range check + de-duplication (build_reference_list, base_model.cpp:27-51)
    c->F_all = p->n_families;
    c->workspace_limit = p->workspace_limit;
    const int T = c->n_taxa;
    const bool may_miss = !device_counts && (p->flags & CAFE_FLAG_MISSING_COUNTS);
    for (int64_t i = 0; !device_counts && i < c->F_all * T; ++i) {
        if (may_miss && p->counts[i] == CAFE_COUNT_MISSING) { c->has_missing = true; continue; }
        if (p->counts[i] < 0 || p->counts[i] > c->M) {
            set_err(c, "cafe_create: family %lld has a count outside [0, %d]", (long long)(i / T), c->M);
            return CAFE_ERR_ARGUMENT;
        }
    }
    c->ref_of.resize(c->F_all);
    if ((p->flags & CAFE_FLAG_NO_DEDUP) || device_counts) {
        uniq.resize(c->F_all);
        for (int64_t f = 0; f < c->F_all; ++f) { uniq[f] = f; c->ref_of[f] = f; }
        c->weights.assign(c->F_all, 1.0);
    } else {
        std::unordered_map<std::string, int64_t> seen;
        seen.reserve((size_t)c->F_all * 2);
        for (int64_t f = 0; f < c->F_all; ++f) {
            std::string key(reinterpret_cast<const char*>(p->counts + f * T), sizeof(int32_t) * T);
            auto it = seen.find(key);
            if (it == seen.end()) {
                seen.emplace(std::move(key), (int64_t)uniq.size());
                c->ref_of[f] = (int64_t)uniq.size();
                uniq.push_back(f);
                c->weights.push_back(1.0);
            } else {
                c->ref_of[f] = it->second;
                c->weights[it->second] += 1.0;
            }
        }
    }
    c->F_uniq = (int64_t)uniq.size();
    c->Fp = round_up64(c->F_uniq, kBN);
    // Columns in order of the families' largest count: a likelihood column is exactly zero far from the observed sizes
    // (node_level_kernel), K2 skips the all-zero rows of a 128-column tile of its B operand, and a tile of families of
    // similar size has many of them.  Internal order only: ref_of maps every family of the table to its column.
    if (!device_counts) {
        std::vector<int32_t> key(c->F_uniq);
        for (int64_t u = 0; u < c->F_uniq; ++u) key[u] = *std::max_element(p->counts + uniq[u] * T, p->counts + (uniq[u] + 1) * T);
        std::vector<int64_t> perm(c->F_uniq), inv(c->F_uniq);
        for (int64_t u = 0; u < c->F_uniq; ++u) perm[u] = u;
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return key[x] < key[y]; });
        std::vector<int64_t> nu(c->F_uniq);
        std::vector<double> nw(c->F_uniq);
        for (int64_t i = 0; i < c->F_uniq; ++i) { nu[i] = uniq[perm[i]]; nw[i] = c->weights[perm[i]]; inv[perm[i]] = i; }
        uniq.swap(nu);
        c->weights.swap(nw);
        for (int64_t f = 0; f < c->F_all; ++f) c->ref_of[f] = inv[c->ref_of[f]];
    }
    return CAFE_OK;
}

template <class T>
int upload(cafe_ctx* c, T** d, const std::vector<T>& h) {
    HIP_TRY(c, hipMalloc(d, sizeof(T) * std::max<size_t>(1, h.size())));
    HIP_TRY(c, hipMemcpy(*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return CAFE_OK;
}

// matrix pools: one slot per (distinct quantized branch length, lambda index) pair and category, per layout.
// Leaf branches use row-major matrices (K3 gathers a column), interior branches k-major ones (K2's A).
void plan_pools(cafe_ctx* c, int kb) {
    c->pair_of.assign(c->n_nodes, -1);
    std::map<std::pair<long, int>, int> seen[2], any;
    for (int v = 0; v < c->n_nodes; ++v) {
        if (v == c->root) continue;
        const int layout = c->leaf_taxon[v] >= 0 ? 0 : 1;
        const long tq = quantize_time(c->blen[v]);
        const auto key = std::make_pair(tq, c->lam_idx[v]);
        auto it = seen[layout].find(key);
        if (it == seen[layout].end()) {
            it = seen[layout].emplace(key, (int)c->pair_tq[layout].size()).first;
            c->pair_tq[layout].push_back(tq);
            c->pair_lam[layout].push_back(c->lam_idx[v]);
        }
        c->pair_of[v] = it->second;
        any.emplace(key, 0);
    }
    c->n_pairs[0] = (int)c->pair_tq[0].size(); c->n_pairs[1] = (int)c->pair_tq[1].size();
    c->n_distinct_pairs = (int)any.size();
    c->kc = round_up(c->M + 1, kBK);
    c->pool = row_major_pool(c->N);
    c->pool.ext_blocks = c->N;               // row-major: one entry per column x of a leaf branch's matrix
    c->max_slots = c->n_pairs[0] * c->Kmax;
    c->kpool.n = c->N; c->kpool.rows = c->kc; c->kpool.k_valid = c->M + 1; c->kpool.kmajor = 1;
    c->kpool.ld = round_up(c->N - 1, 16) + round_up(kMaxBM, 16) + 16;     // a row tile may start at any valid row
    c->kpool.stride = (int64_t)c->kc * c->kpool.ld;
    c->kpool.ext_blocks = (c->N - 1 + 15) / 16;
    c->max_kslots = c->n_pairs[1] * c->Kmax;
    c->slot_of.assign((size_t)c->n_nodes * c->Kmax, -1);
    for (int v = 0; v < c->n_nodes; ++v) {
        if (v == c->root) continue;
        const int layout = c->leaf_taxon[v] >= 0 ? 0 : 1;
        for (int k = 0; k < c->Kmax; ++k) c->slot_of[(size_t)v * c->Kmax + k] = k * c->n_pairs[layout] + c->pair_of[v];
    }
    // small matrices (a K2 launch is one round of tiles and lasts as long as one tile): 16-deep K tiles, half as many DMA
    // round trips per tile; otherwise 12-deep ones: still four workgroups per CU, a third fewer barriers per MFMA than 8-deep
    // ones (config 4: 130.4 against 133.6 ms per call)
    c->kb = kb ? kb : (c->N < 256 ? 16 : 12);
    // likelihood panels: rows padded so that every panel can be a GEMM B operand (kc rows) or the root (R rows)
    // a factor GEMM stores transposed, [column][16 - out_off + panel row] (prune_gemm.hip): factor_ld rows per column, and a
    // panel slot must be able to hold a factor of as many columns
    c->factor_ld = round_up(std::max(c->M + 1, c->R) + 16, 16);
    c->rows_pad = std::max(std::max(c->kc, round_up(c->R, kBK)), c->factor_ld);
}

// The family table on the device (counts taxon-major, padded families replicate an all-zero family) and the subtree
// pattern tables when plan_patterns built them (the host copies are released)
int upload_families(cafe_ctx* c, const cafe_problem* p, const std::vector<int64_t>& uniq) {
    const int T = c->n_taxa;
    std::vector<int32_t> tm((size_t)T * c->Fp, 0);
    for (int64_t u = 0; !(p->flags & kFlagDeviceCounts) && u < c->F_uniq; ++u)
        for (int t = 0; t < T; ++t) tm[(size_t)t * c->Fp + u] = p->counts[uniq[u] * T + t];
    std::vector<double> w(c->Fp, 0.0);
    std::copy(c->weights.begin(), c->weights.end(), w.begin());
    if (int rc = upload(c, &c->d_counts, tm)) return rc;
    if (int rc = upload(c, &c->d_weights, w)) return rc;
    c->d_leaf_cnt.assign(c->h_leaf_cnt.size(), nullptr); c->d_edge_map.assign(c->h_edge_map.size(), nullptr);
    for (size_t v = 0; v < c->h_leaf_cnt.size(); ++v) {
        if (!c->h_leaf_cnt[v].empty()) if (int rc = upload(c, &c->d_leaf_cnt[v], c->h_leaf_cnt[v])) return rc;
        for (int u : c->inner[v]) if (!c->h_edge_map[u].empty()) if (int rc = upload(c, &c->d_edge_map[u], c->h_edge_map[u])) return rc;
    }
    c->h_leaf_cnt.clear(); c->h_edge_map.clear();
    return CAFE_OK;
}

// What lives as long as the context beside the family table: the matrix pools, the per-call parameter block, the outputs
int alloc_resident(cafe_ctx* c, bool kskip, bool gemm_stamps) {
    const size_t pool_bytes = (size_t)std::max(1, c->max_slots) * c->pool.stride * sizeof(double);
    const size_t kpool_bytes = (size_t)std::max(1, c->max_kslots) * c->kpool.stride * sizeof(double);
    if (hipMalloc(&c->pool.base, pool_bytes) != hipSuccess || hipMalloc(&c->kpool.base, kpool_bytes) != hipSuccess) {
        set_err(c, "cafe_create: cannot allocate %.2f GB for %d transition matrices of order %d", (pool_bytes + kpool_bytes) / 1e9,
                c->max_slots + c->max_kslots, c->N);
        return CAFE_ERR_MEMORY;
    }
    // padding columns / rows of both layouts are never written by K1 and must read as 0
    HIP_TRY(c, hipMemset(c->pool.base, 0, pool_bytes));
    HIP_TRY(c, hipMemset(c->kpool.base, 0, kpool_bytes));
    // non-zero extents of the matrices (K1 writes them, K2 skips the K tiles outside them), and the host copy of the
    // k-major ones that picks K2's tile heights
    if (kskip) {
        HIP_TRY(c, hipMalloc(&c->kpool.ext, sizeof(int32_t) * 2 * (size_t)std::max(1, c->max_kslots) * c->kpool.ext_blocks));
        HIP_TRY(c, hipMemset(c->kpool.ext, 0, sizeof(int32_t) * 2 * (size_t)std::max(1, c->max_kslots) * c->kpool.ext_blocks));
        HIP_TRY(c, hipMalloc(&c->pool.ext, sizeof(int32_t) * 2 * (size_t)std::max(1, c->max_slots) * c->pool.ext_blocks));
        HIP_TRY(c, hipMemset(c->pool.ext, 0, sizeof(int32_t) * 2 * (size_t)std::max(1, c->max_slots) * c->pool.ext_blocks));
        HIP_TRY(c, hipHostMalloc(&c->h_ext, sizeof(int32_t) * 2 * (size_t)std::max(1, c->max_kslots) * c->kpool.ext_blocks, hipHostMallocDefault));
    }
    c->stats.matrix_bytes = (int64_t)(pool_bytes + kpool_bytes);
    // per-call parameter block (layout: cafe_ctx.h), device + pinned mirror
    size_t off = sizeof(SlotParam) * (size_t)(c->max_slots + c->max_kslots);
    off = (off + 63) / 64 * 64;
    const size_t off_prior = off; off += sizeof(double) * c->R;
    const size_t off_logprior = off; off += sizeof(double) * c->R;
    const size_t off_cat = off; off += sizeof(double) * c->Kmax;
    const size_t off_err = off; off += sizeof(double) * (size_t)(c->M + 1) * std::max(1, c->n_dev);
    c->params_bytes = off;
    HIP_TRY(c, hipMalloc(&c->d_params, c->params_bytes));
    HIP_TRY(c, hipMemset(c->d_params, 0, c->params_bytes));
    c->d_slots = reinterpret_cast<SlotParam*>(c->d_params);
    c->d_prior = reinterpret_cast<double*>(c->d_params + off_prior);
    c->d_logprior = reinterpret_cast<double*>(c->d_params + off_logprior);
    c->d_catprobs = reinterpret_cast<double*>(c->d_params + off_cat);
    c->d_err = c->n_dev > 0 ? reinterpret_cast<double*>(c->d_params + off_err) : nullptr;
    c->stage_bytes = c->params_bytes;
    HIP_TRY(c, hipHostMalloc(&c->h_stage, c->stage_bytes, hipHostMallocDefault));
    std::memset(c->h_stage, 0, c->stage_bytes);
    HIP_TRY(c, hipHostMalloc(&c->h_result, 4 * sizeof(double), hipHostMallocDefault));
    c->h_poison = c->h_result + 2;                       // what a failing rank of a communicator feeds the all-reduce
    c->h_poison[0] = 0.0; c->h_poison[1] = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_upload, hipEventDisableTiming));
    for (auto& e : c->ev) HIP_TRY(c, hipEventCreate(&e));
    hipDeviceProp_t prop;
    HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
    c->n_cu = prop.multiProcessorCount;
    // outputs
    HIP_TRY(c, hipMalloc(&c->d_fam_out, sizeof(double) * c->Fp));
    HIP_TRY(c, hipMalloc(&c->d_fam_lik, sizeof(double) * c->Fp));
    HIP_TRY(c, hipMalloc(&c->d_cat_out, sizeof(double) * c->Fp * c->Kmax));
    HIP_TRY(c, hipMalloc(&c->d_failed, sizeof(int32_t) * c->Fp));
    HIP_TRY(c, hipMemset(c->d_failed, 0, sizeof(int32_t) * c->Fp));
    HIP_TRY(c, hipMalloc(&c->d_scratch, sizeof(double) * (2 * c->n_scratch + 1)));      // partials + the ticket counter of the final sum
    HIP_TRY(c, hipMemset(c->d_scratch, 0, sizeof(double) * (2 * c->n_scratch + 1)));
    HIP_TRY(c, hipMalloc(&c->d_result, sizeof(double) * 2));
    if (gemm_stamps) {
        c->stamps_words = (size_t)6 * 8 * ((c->Fp / kBN + 8) * 16) * c->Kmax;
        HIP_TRY(c, hipMalloc(&c->d_stamps, c->stamps_words * sizeof(unsigned long long)));
        HIP_TRY(c, hipMemset(c->d_stamps, 0, c->stamps_words * sizeof(unsigned long long)));
    }
    return CAFE_OK;
}

// a leaf child's row in the counts its parent's ops read (the parent's pattern table, or the family table)
int cnt_row(const cafe_ctx* c, int leaf) { return c->subtree_dedup ? c->leaf_rank[leaf] : c->leaf_taxon[leaf]; }

// The arena of the likelihood panels, and the zero extents of the planned nodes' panels with their descriptors
int alloc_panels(cafe_ctx* c, size_t panel_doubles, const std::vector<int>& ext_order, bool magskip) {
    // (+64 KB: the assemble pass reads whole 64-row tiles of a transposed factor, up to a tile past its last column)
    const size_t panel_bytes = panel_doubles * sizeof(double) + 65536;
    if (hipMalloc(&c->d_panels, panel_bytes) != hipSuccess) { set_err(c, "cafe_create: cannot allocate %.2f GB of likelihood panels", panel_bytes / 1e9); return CAFE_ERR_MEMORY; }
    // rows beyond what the first writer of a panel covers must not hold NaN bit patterns
    HIP_TRY(c, hipMemset(c->d_panels, 0, panel_bytes));
    c->stats.panel_bytes = (int64_t)panel_bytes; c->stats.n_unique_families = c->F_uniq;
    c->d_colext.assign(c->n_nodes, nullptr); c->d_tileext.assign(c->n_nodes, nullptr); c->d_narrow.assign(c->n_nodes, nullptr);
    for (int v : ext_order) {
        const int64_t cols = panel_cols(c, v, c->Fp);
        HIP_TRY(c, hipMalloc(&c->d_colext[v], sizeof(int32_t) * 2 * (size_t)c->Kmax * cols));
        HIP_TRY(c, hipMalloc(&c->d_tileext[v], sizeof(int32_t) * 2 * (size_t)c->Kmax * (cols / kBN)));
        HIP_TRY(c, hipMalloc(&c->d_narrow[v], sizeof(int32_t) * 2 * (size_t)c->Kmax * (cols / kBN)));
    }
    // magnitude tables and panel bounds (extents.hip).  They come after the panels and are an optimisation: where they do
    // not fit, the call keeps the exact extents.
    c->d_bound.assign(c->n_nodes, nullptr);
    c->n_ksteps = (c->M + 1 + 3) / 4; c->n_rsteps = (c->N + 3) / 4;
    if (c->panel_extents && magskip) {
        bool ok = hipMalloc(&c->d_mag_a16, sizeof(int32_t) * (size_t)c->max_kslots * c->n_ksteps * c->kpool.ext_blocks) == hipSuccess &&
                  hipMalloc(&c->d_mag_t4, sizeof(int32_t) * (size_t)c->max_kslots * c->n_ksteps * c->n_rsteps) == hipSuccess &&
                  hipMalloc(&c->d_mag_lt, sizeof(int32_t) * (size_t)std::max(1, c->max_slots) * (c->M + 1) * c->n_rsteps) == hipSuccess;
        for (int v : ext_order)
            ok = ok && hipMalloc(&c->d_bound[v], sizeof(int32_t) * (size_t)c->Kmax * (panel_cols(c, v, c->Fp) / kBN) * c->n_rsteps) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        c->magskip = ok;
    }
    if (c->panel_extents) {
        std::vector<ExtNode> nodes;
        for (int v : ext_order) {
            ExtNode nd{};
            nd.bound = c->magskip ? c->d_bound[v] : nullptr;
            nd.cols = (int32_t)panel_cols(c, v, c->Fp);
            nd.colext = c->d_colext[v]; nd.tileext = c->d_tileext[v]; nd.narrow = c->d_narrow[v];
            nd.cnt = c->subtree_dedup ? c->d_leaf_cnt[v] : c->d_counts; nd.cnt_ld = nd.cols;
            for (int u : c->leaves[v]) { nd.leaf_pair[nd.n_leaf] = c->pair_of[u]; nd.leaf_row[nd.n_leaf++] = cnt_row(c, u); }
            for (int u : c->inner[v]) {
                nd.inner_pair[nd.n_inner] = c->pair_of[u];
                nd.inner_cols[nd.n_inner] = (int32_t)panel_cols(c, u, c->Fp);
                nd.inner_map[nd.n_inner] = c->subtree_dedup ? c->d_edge_map[u] : nullptr;    // (nullptr for an identity edge)
                nd.inner_bound[nd.n_inner] = c->magskip ? c->d_bound[u] : nullptr;
                nd.inner_narrow[nd.n_inner] = c->d_narrow[u];
                nd.inner_colext[nd.n_inner++] = c->d_colext[u];
            }
            nodes.push_back(nd);
        }
        return upload(c, &c->d_ext_nodes, nodes);
    }
    return CAFE_OK;
}

// Static descriptors (n_row_tiles of a K2 op follows the tile height, chosen per call) and the per-call launch state
int build_descriptors(cafe_ctx* c, const std::vector<int>& lt_of_pair) {
    c->h_gemm_ops.assign(std::max(1, c->n_gemm_ops), GemmOp{}); c->h_gather_ops.assign(std::max(1, c->n_gather_ops), GatherArgs{});
    // joint K ranges of the K2 ops (whenever the matrices publish extents): per op [category][column tiles or 1][blocks + pad]
    const size_t jr_row = (size_t)c->kpool.ext_blocks + kRangePad;
    if (c->kpool.ext) {
        size_t words = 0;
        for (const Op& op : c->ops)
            if (op.type == 1) words += (size_t)c->Kmax * (c->panel_extents ? panel_cols(c, op.child, c->Fp) / kBN : 1) * jr_row;
        HIP_TRY(c, hipMalloc(&c->d_jr, sizeof(int32_t) * std::max<size_t>(1, words)));
    }
    size_t jr_used = 0;
    const int64_t lt_kstride = (int64_t)(c->M + 1) * c->factor_ld;
    for (const Op& op : c->ops) {
        const int32_t* cnt_base = c->subtree_dedup ? c->d_leaf_cnt[op.parent] : c->d_counts;
        const int64_t cnt_ld = panel_cols(c, op.parent, c->Fp);
        const Panel& D = c->panels[op.dst_panel];
        if (op.type == 1) {
            GemmOp& g = c->h_gemm_ops[op.desc];
            const Panel& S = c->panels[op.src_panel];
            for (int k = 0; k < c->Kmax; ++k) g.slot[k] = c->slot_of[(size_t)op.child * c->Kmax + k];
            g.src = c->d_panels + S.offset; g.src_kstride = S.kstride;
            g.dst = c->d_panels + D.offset; g.dst_kstride = D.kstride;
            g.ld = (int32_t)panel_cols(c, op.child, c->Fp);               // the GEMM runs over the child's columns (= the parent's when direct)
            g.n_col_tiles = g.ld / kBN;
            g.rows = op.to_root ? c->R : c->M;               // parent sizes 1..rows
            g.out_off = op.to_root ? 0 : 1; g.dst_ldt = op.to_factor ? c->factor_ld : 0; g.n_leaf = op.n_leaf;
            if (op.n_leaf) {
                g.taxon = cnt_row(c, op.leaf_node[0]);
                for (int k = 0; k < c->Kmax; ++k) g.leaf_slot[k] = c->slot_of[(size_t)op.leaf_node[0] * c->Kmax + k];
            }
            g.counts = cnt_base; g.counts_ld = cnt_ld;
            if (op.has_gath) {
                const Panel& G = c->panels[op.gath_panel];
                g.gath_src = c->d_panels + G.offset; g.gath_kstride = G.kstride;
                g.gath_ld = c->factor_ld; g.gath_map = c->d_edge_map[op.gath_child];
            }
            g.bext = c->panel_extents ? c->d_tileext[op.child] : nullptr;
            if (c->d_jr) {
                g.jr = c->d_jr + jr_used;
                g.jr_nct = c->panel_extents ? g.n_col_tiles : 1; g.jr_ct_mask = c->panel_extents ? -1 : 0;
                jr_used += (size_t)c->Kmax * g.jr_nct * jr_row;
                c->jr_max_tiles = std::max(c->jr_max_tiles, (int)g.jr_nct);
                g.bbound = c->magskip ? c->d_bound[op.child] : nullptr;
                g.bnarrow = c->magskip && c->panel_extents ? c->d_narrow[op.child] : nullptr;
            }
        } else {
            GatherArgs& g = c->h_gather_ops[op.desc];
            g.n_leaf = op.n_leaf;
            for (int l = 0; l < op.n_leaf; ++l) {
                g.taxon[l] = cnt_row(c, op.leaf_node[l]);
                for (int k = 0; k < c->Kmax; ++k) g.slot[l][k] = c->slot_of[(size_t)op.leaf_node[l] * c->Kmax + k];
            }
            g.counts = cnt_base; g.counts_ld = cnt_ld;
            g.dst = c->d_panels + D.offset; g.panel_kstride = D.kstride; g.ld = (int32_t)panel_cols(c, op.parent, c->Fp);
            g.row_off = op.to_root ? 1 : 0; g.rows = op.to_root ? c->R : c->M + 1; g.rows_store = op.to_root ? c->R : c->kc;
            g.mode = op.mode; g.n_src = op.n_src;
            for (int j = 0; j < op.n_src; ++j) {
                const Panel& S = c->panels[op.src_panels[j]];
                g.src[j] = c->d_panels + S.offset; g.kstride_src[j] = S.kstride;
                g.ld_src[j] = c->factor_ld; g.map[j] = c->d_edge_map[op.src_child[j]];
            }
            // (the root's vector is read whole by the reduction and has no extent record)
            // (the narrowed hull: it is the structural one in a call without magnitude tables, and no K range reaches outside it)
            g.tileext = c->panel_extents && !op.to_root && !c->no_asm_skip ? c->d_narrow[op.parent] : nullptr;
            g.lt_kstride = lt_kstride;
            if (op.leaf_t)
                for (int l = 0; l < op.n_leaf && l < kMaxLeafPerOp; ++l)
                    g.lt[l] = c->d_lt + (int64_t)lt_of_pair[c->pair_of[op.leaf_node[l]]] * c->Kmax * lt_kstride;
        }
    }
    if (int rc = upload(c, &c->d_gather_ops, c->h_gather_ops)) return rc;
    HIP_TRY(c, hipHostMalloc(&c->h_gemm_stage, sizeof(GemmOp) * c->h_gemm_ops.size(), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc(&c->h_plan_desc, sizeof(PlanLaunch) * std::max(1, c->n_gemm_groups), hipHostMallocDefault));
    c->gemm_ev.resize((size_t)2 * c->n_gemm_groups * c->stats.n_chunks);
    for (auto& e : c->gemm_ev) HIP_TRY(c, hipEventCreate(&e));
    return CAFE_OK;
}

}  // namespace

int create_impl(cafe_ctx* c, const cafe_problem* p) {
    const Switches sw = read_switches(c);
    std::vector<int64_t> uniq;
    int rc = load_problem(c, p, uniq);
    if (rc != CAFE_OK) return rc;
    const bool device_counts = p->flags & kFlagDeviceCounts;      // internal: the caller fills d_counts on the device
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err(c, "cafe_create: no HIP device available (this library has no CPU path)"); return CAFE_ERR_DEVICE; }
    if (c->device < 0 || c->device >= ndev) { set_err(c, "cafe_create: device %d out of range (%d devices)", c->device, ndev); return CAFE_ERR_DEVICE; }
    HIP_TRY(c, hipSetDevice(c->device));
    c->device_ready = true;
    HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));

    // subtree-level de-duplication tables (the schedule depends on them)
    const bool dedup = !device_counts && !(p->flags & CAFE_FLAG_NO_SUBTREE_DEDUP);
    if (dedup) plan_patterns(c, p, uniq, !sw.no_cherry_swap, sw.inherit_all, sw.inherit_big);
    if ((rc = upload_families(c, p, uniq)) != CAFE_OK) return rc;
    plan_pools(c, sw.kb);
    // Extents (K2 skips the K tiles outside a matrix's non-zero band).  Small matrices (mammals: N = 141, 9 K tiles): a row
    // tile spans most of the band anyway, and the extent kernels and lookups cost more than the few K tiles they would save
    // (measured: 0.34 -> 0.38 ms per call with them) -- no extents below N = 256
    const bool kskip = !sw.no_kskip && c->N >= 256;
    if ((rc = alloc_resident(c, kskip, sw.gemm_stamps)) != CAFE_OK) return rc;

    // the schedule, for a panel budget of what is free now (or the given workspace)
    size_t budget = 0;
    if ((rc = panel_budget(c, &budget)) != CAFE_OK) return rc;
    // K2 addresses a panel category through a 32-bit buffer descriptor: rows_pad * cols * 8 bytes must stay below 4 GB
    const int64_t desc_cols = (int64_t)(0xFFFFFFF0ll / ((int64_t)c->rows_pad * 8)) / kBN * kBN;
    const size_t panel_doubles = plan_schedule(c, dedup, !sw.no_groups, budget, desc_cols);
    if (c->chunk_cols < kBN) { set_err(c, "cafe_create: %zu bytes of workspace cannot hold %d panels of one 128-family tile", budget, c->n_panels); return CAFE_ERR_MEMORY; }
    const std::vector<int> ext_order = plan_extent_levels(c, kskip);
    if ((rc = alloc_panels(c, panel_doubles, ext_order, !sw.no_magskip)) != CAFE_OK) return rc;

    // transposed leaf copies, if they fit what is free after the panels
    std::vector<int> lt_of_pair;
    if (!sw.no_leaf_t) {
        size_t free_now = 0, total_now = 0;
        HIP_TRY(c, hipMemGetInfo(&free_now, &total_now));
        if (const size_t lt_bytes = plan_leaf_transposes(c, sw.lt_min, free_now, lt_of_pair)) {
            HIP_TRY(c, hipMalloc(&c->d_lt, lt_bytes));
            HIP_TRY(c, hipMemset(c->d_lt, 0, lt_bytes));
            if ((rc = upload(c, &c->d_lt_pairs, c->lt_pairs)) != CAFE_OK) return rc;
        }
    }

    group_launches(c);
    if ((rc = build_descriptors(c, lt_of_pair)) != CAFE_OK) return rc;
    if (sw.dump_schedule) dump_schedule(c);
    HIP_TRY(c, hipDeviceSynchronize());
    return CAFE_OK;
}

cafe_ctx* create_child_for_device_counts(const cafe_ctx* parent, int64_t n_families) {
    cafe_ctx* c = new (std::nothrow) cafe_ctx();
    if (!c) return nullptr;
    cafe_problem pb{};
    std::vector<int32_t> par(parent->parent.begin(), parent->parent.end()), lam(parent->lam_idx.begin(), parent->lam_idx.end()),
        leaf(parent->leaf_taxon.begin(), parent->leaf_taxon.end());
    pb.n_nodes = parent->n_nodes; pb.parent = par.data(); pb.branch_length = parent->blen.data(); pb.lambda_index = lam.data();
    pb.leaf_taxon = leaf.data(); pb.n_taxa = parent->n_taxa; pb.n_families = n_families; pb.counts = nullptr;
    pb.max_family_size = parent->M; pb.max_root_family_size = parent->R; pb.n_lambdas = parent->n_lambdas;
    pb.single_lambda = parent->single_lambda; pb.max_categories = 1; pb.n_deviations = 0; pb.device = parent->device;
    pb.flags = kFlagDeviceCounts; pb.workspace_limit = 0;
    if (guarded(c, "cafe_create", [&] { return create_impl(c, &pb); }) != CAFE_OK) { free_device(c); delete c; return nullptr; }
    return c;
}

void destroy_child(cafe_ctx* c) {
    if (!c) return;
    free_device(c);
    delete c;
}

}  // namespace cafe

extern "C" {

int cafe_abi_version(void) { return CAFE_ABI_VERSION; }

cafe_ctx* cafe_create(const cafe_problem* problem, char* err, size_t errlen) {
    cafe_ctx* c = new (std::nothrow) cafe_ctx();
    if (!c) return nullptr;
    const int rc = guarded(c, "cafe_create", [&]() -> int {
        if (problem && (problem->flags & kFlagDeviceCounts)) { set_err(c, "cafe_create: unknown flag"); return CAFE_ERR_ARGUMENT; }
        return create_impl(c, problem);
    });
    if (rc != CAFE_OK) {
        if (err && errlen) { std::snprintf(err, errlen, "%s", c->err.c_str()); }
        free_device(c);
        delete c;
        return nullptr;
    }
    if (err && errlen) err[0] = 0;
    return c;
}

void cafe_destroy(cafe_ctx* ctx) {
    if (!ctx) return;
    free_device(ctx);
    delete ctx;
}

const char* cafe_last_error(const cafe_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int cafe_matrix_size(const cafe_ctx* ctx) { return ctx ? ctx->N : 0; }

}  // extern "C"
