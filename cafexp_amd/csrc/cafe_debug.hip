// Diagnostics and read-backs of the C ABI: what the last call built and ran (matrices, extents, tile lists, executed
// flops, launch times), the test hooks, and the two context-free probes.  Nothing here is on the scorer path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cafe_call.h"

using namespace cafe;

namespace cafe {

// The joint K ranges of a K2 op as the last call's range_kernel left them: [K][g.jr_nct][ext_blocks + kRangePad] (empty: none)
static bool read_ranges(cafe_ctx* c, const GemmOp& g, int K, std::vector<int32_t>& out) {
    out.clear();
    if (!g.jr) return true;
    out.resize((size_t)K * g.jr_nct * (c->kpool.ext_blocks + kRangePad));
    return hipMemcpy(out.data(), g.jr, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess;
}

// The same table from the exact-zero extents alone (range_kernel without magnitude tables, on the host): what the ranges
// are under CAFE_NO_MAGSKIP=1, whatever the last call used.  aext: the k-major pool's extents, read back by the caller.
static bool exact_ranges(cafe_ctx* c, const GemmOp& g, int K, const std::vector<int32_t>& aext, std::vector<int32_t>& out) {
    out.clear();
    if (!g.jr) return true;
    const int nb = c->kpool.ext_blocks, row = nb + kRangePad;
    out.assign((size_t)K * g.jr_nct * row, 1);             // lo 1, hi 0: none
    std::vector<int32_t> bext;
    if (g.bext) {
        bext.resize((size_t)2 * K * g.jr_nct);
        if (hipMemcpy(bext.data(), g.bext, bext.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
    }
    for (int k = 0; k < K; ++k)
        for (int ct = 0; ct < g.jr_nct; ++ct) {
            int plo = 0, phi = c->M;
            if (g.bext) {
                const int32_t* be = bext.data() + ((size_t)k * g.jr_nct + ct) * 2;
                plo = be[0]; phi = std::min(be[1], phi);
                if (be[1] < be[0]) { plo = 0; phi = 0; }    // an empty panel extent: row 0 (extents.hip)
            }
            for (int b = 0; b < nb; ++b) {
                const int32_t* e = aext.data() + ((size_t)g.slot[k] * nb + b) * 2;
                const int lo = std::max(e[0], plo), hi = std::min(e[1], phi);
                if (hi >= lo) out[((size_t)k * g.jr_nct + ct) * row + b] = (lo / 4) | ((hi / 4) << 16);
            }
        }
    return true;
}

// K range of a row tile = hull of its blocks' joint ranges.  e: the `mi` 16-row blocks of the tile in a row of a range table, each
// first | last << 16 in 4-deep k-steps, first > last: none.  false (and an empty hull, *slo > *shi): no block has a range.
static bool tile_k_hull(const int32_t* e, int mi, int* slo, int* shi) {
    *slo = 0x7fff; *shi = -1;
    for (int b = 0; b < mi; ++b)
        if ((e[b] >> 16) >= (e[b] & 0xFFFF)) { *slo = std::min(*slo, e[b] & 0xFFFF); *shi = std::max(*shi, e[b] >> 16); }
    return *shi >= *slo;
}

// Flops the K2 launches of the last (profiled) call EXECUTED: a row block of a (row tile, column tile) pair issues MFMAs only
// in the k-steps of its joint range (GemmOp::jr: matrix extent x panel extent, less the k-steps whose products underflow), so
// read the ranges this call published and count, per launch, what its tiles ran.  A few synchronous copies, milliseconds of
// host work: for measurement, once, not per call.
// per_block: what the kernel issues (prune_gemm.hip block_ranges); false: every block over its tile's whole K range (the hull
// of its blocks' ranges in whole K tiles -- the count of rounds 2 and 3a, kept for comparison).  Both count the valid k and rows only
// (a ragged last k-step counts its k <= M, a ragged last block its rows).
// exact: count over the ranges the exact-zero extents alone give (exact_ranges) -- the products that have no exact zero in
// them, whether or not the call issued them all.
double count_executed_flops(cafe_ctx* c, std::vector<double>* per_launch, bool per_block, bool exact) {
    if (c->gemm_launches_info.empty()) return c->stats.gemm_flops;
    const int kBK = c->kb;
    const int jr_row = c->kpool.ext_blocks + kRangePad;
    double executed = 0;
    std::vector<int32_t> jr, aext;
    if (exact && c->kpool.ext) {
        aext.resize((size_t)2 * c->max_kslots * c->kpool.ext_blocks);
        if (hipMemcpy(aext.data(), c->kpool.ext, aext.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
    }
    for (const auto& L : c->gemm_launches_info) {
        const double before = executed;
        const int mi = L.mi, bm = 16 * mi;
        for (int oi : c->groups[L.group].ops) {
            const Op& op = c->ops[oi];
            const GemmOp& g = c->h_gemm_ops[op.desc];
            const int rows = op.to_root ? c->R : c->M;
            const int64_t cols = panel_cols(c, op.child, L.cols);
            const int n_ct = (int)(cols / kBN);
            if (!(exact ? exact_ranges(c, g, L.K, aext, jr) : read_ranges(c, g, L.K, jr))) return -1.0;
            const bool per_tile = g.jr && g.jr_ct_mask;      // the ranges differ between column tiles
            for (int k = 0; k < L.K; ++k)
                for (int row0 = 0; row0 < rows; row0 += bm)
                    for (int ct = 0; ct < (per_tile ? n_ct : 1); ++ct) {
                        const double width = per_tile ? (double)kBN : (double)cols;
                        const int32_t* e = g.jr ? jr.data() + ((size_t)k * g.jr_nct + ct) * jr_row : nullptr;
                        int slo = 0, shi = c->M / 4;             // no ranges: every k-step
                        if (e && !tile_k_hull(e + row0 / 16, mi, &slo, &shi)) { slo = 0; shi = 0; }     // an all-zero tile runs one K tile
                        const int t_lo = slo * 4 / kBK, t_hi = std::min(shi * 4 + 3, c->M) / kBK;
                        for (int b = row0 / 16; b < row0 / 16 + mi && b * 16 < rows; ++b) {
                            int kk;
                            if (e && per_block) {
                                const int l = e[b] & 0xFFFF, h = e[b] >> 16;
                                if (h < l) continue;
                                kk = std::min((h - l + 1) * 4, c->M + 1 - l * 4);
                            } else {
                                kk = std::min((t_hi - t_lo + 1) * kBK, c->M + 1 - t_lo * kBK);
                            }
                            executed += 2.0 * std::min(16, rows - b * 16) * (double)kk * width;
                        }
                    }
        }
        if (per_launch) per_launch->push_back(executed - before);
    }
    return executed;
}

}  // namespace cafe

extern "C" {

int cafe_debug_fail_next(cafe_ctx* ctx, int n) {
    if (!ctx || n < 0) return CAFE_ERR_ARGUMENT;
    ctx->debug_fail_in = n;
    return CAFE_OK;
}

int cafe_debug_stamps(cafe_ctx* ctx, unsigned long long* out, size_t words) {
    if (!ctx || !ctx->d_stamps || !out) return CAFE_ERR_STATE;
    if (words > ctx->stamps_words) words = ctx->stamps_words;
    return hipMemcpy(out, ctx->d_stamps, words * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? CAFE_OK : CAFE_ERR_DEVICE;
}

int cafe_debug_force_tile(cafe_ctx* ctx, int mi) {
    if (!ctx || (mi != 0 && (mi < 2 || mi > 9))) return CAFE_ERR_ARGUMENT;
    ctx->force_mi = mi;
    return CAFE_OK;
}

int cafe_debug_level_tiles(cafe_ctx* ctx, int tiles) {
    if (!ctx || (tiles != 0 && tiles != 1 && tiles != 2 && tiles != 4)) return CAFE_ERR_ARGUMENT;
    ctx->force_level_tiles = tiles;
    return CAFE_OK;
}

int cafe_get_extents(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* matrix_ext, size_t matrix_ext_len,
                     int32_t* panel_ext, size_t panel_ext_len, int32_t* n_tiles) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_get_extents")) return rc;
    if (node < 0 || node >= ctx->n_nodes || node == ctx->root || category < 0 || category >= ctx->last.K) {
        set_err(ctx, "cafe_get_extents: node/category out of range");
        return CAFE_ERR_ARGUMENT;
    }
    if (!ctx->kpool.ext || !ctx->pool.ext) { set_err(ctx, "cafe_get_extents: extents are switched off"); return CAFE_ERR_STATE; }
    if (const int rc = wait_last_call(ctx)) return rc;
    const bool leaf = ctx->leaf_taxon[node] >= 0;
    const MatrixPool& mp = leaf ? ctx->pool : ctx->kpool;
    const int slot = ctx->slot_of[(size_t)node * ctx->Kmax + category];
    if (matrix_ext) {
        if (matrix_ext_len < (size_t)2 * mp.ext_blocks) { set_err(ctx, "cafe_get_extents: matrix_ext too small"); return CAFE_ERR_ARGUMENT; }
        HIP_TRY(ctx, hipMemcpy(matrix_ext, mp.ext + (size_t)slot * mp.ext_blocks * 2, sizeof(int32_t) * 2 * mp.ext_blocks, hipMemcpyDeviceToHost));
    }
    if (n_tiles) *n_tiles = 0;
    if (panel_ext && !leaf && ctx->panel_extents && ctx->d_tileext[node]) {
        const int nt = (int)(panel_cols(ctx, node, ctx->Fp) / kBN);
        if (panel_ext_len < (size_t)2 * nt) { set_err(ctx, "cafe_get_extents: panel_ext too small"); return CAFE_ERR_ARGUMENT; }
        HIP_TRY(ctx, hipMemcpy(panel_ext, ctx->d_tileext[node] + (size_t)category * nt * 2, sizeof(int32_t) * 2 * nt, hipMemcpyDeviceToHost));
        if (n_tiles) *n_tiles = nt;
    }
    return CAFE_OK;
}

int cafe_debug_leaf_transposes(cafe_ctx* ctx, int32_t* n_branches, int32_t* used_by_last_call) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (n_branches) *n_branches = ctx->d_lt ? (int32_t)ctx->lt_pairs.size() : 0;
    if (used_by_last_call) *used_by_last_call = ctx->last.leaf_t ? 1 : 0;
    return CAFE_OK;
}

int cafe_debug_column_extents(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* out, size_t out_len, int64_t* n_cols) {
    if (!ctx || !out) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_debug_column_extents")) return rc;
    if (node < 0 || node >= ctx->n_nodes || category < 0 || category >= ctx->last.K || !ctx->panel_extents || !ctx->d_colext[node]) {
        set_err(ctx, "cafe_debug_column_extents: no extents for this node");
        return CAFE_ERR_ARGUMENT;
    }
    const int64_t cols = panel_cols(ctx, node, ctx->Fp);
    if (n_cols) *n_cols = cols;
    if (out_len < (size_t)2 * cols) { set_err(ctx, "cafe_debug_column_extents: out too small"); return CAFE_ERR_ARGUMENT; }
    if (const int rc = wait_last_call(ctx)) return rc;
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_colext[node] + (size_t)category * cols * 2, sizeof(int32_t) * 2 * cols, hipMemcpyDeviceToHost));
    return CAFE_OK;
}

// Upper bounds of a node's panel (node_level_kernel): out[tile * row_steps + r] = bound of log2 of every computed entry of
// rows 4 r .. 4 r + 3 in 128-column tile `tile` of `category`; -inf where all of them are exactly zero.
int cafe_debug_panel_bounds(cafe_ctx* ctx, int32_t node, int32_t category, double* out, size_t out_len, int32_t* n_tiles, int32_t* row_steps) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_debug_panel_bounds")) return rc;
    if (node < 0 || node >= ctx->n_nodes || category < 0 || category >= ctx->last.K) { set_err(ctx, "cafe_debug_panel_bounds: node/category out of range"); return CAFE_ERR_ARGUMENT; }
    if (!ctx->last.magskip || !ctx->d_bound[node]) { set_err(ctx, "cafe_debug_panel_bounds: the last call kept no bounds for this node"); return CAFE_ERR_STATE; }
    const int nt = (int)(panel_cols(ctx, node, ctx->Fp) / kBN), nr = ctx->n_rsteps;
    if (n_tiles) *n_tiles = nt;
    if (row_steps) *row_steps = nr;
    if (!out) return CAFE_OK;
    if (out_len < (size_t)nt * nr) { set_err(ctx, "cafe_debug_panel_bounds: out too small"); return CAFE_ERR_ARGUMENT; }
    if (const int rc = wait_last_call(ctx)) return rc;
    std::vector<int32_t> q((size_t)nt * nr);
    HIP_TRY(ctx, hipMemcpy(q.data(), ctx->d_bound[node] + (size_t)category * nt * nr, q.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < q.size(); ++i) out[i] = q[i] == kMagNone ? -HUGE_VAL : (double)q[i] / kMagUnit;
    return CAFE_OK;
}

// The narrowed hulls of a node's panel (node_level_kernel, ExtNode::narrow): out[tile][2]
int cafe_debug_narrowed_extents(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* out, size_t out_len, int32_t* n_tiles) {
    if (!ctx || !out) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_debug_narrowed_extents")) return rc;
    if (node < 0 || node >= ctx->n_nodes || category < 0 || category >= ctx->last.K || !ctx->panel_extents || !ctx->d_narrow[node]) {
        set_err(ctx, "cafe_debug_narrowed_extents: no extents for this node");
        return CAFE_ERR_ARGUMENT;
    }
    const int nt = (int)(panel_cols(ctx, node, ctx->Fp) / kBN);
    if (n_tiles) *n_tiles = nt;
    if (out_len < (size_t)2 * nt) { set_err(ctx, "cafe_debug_narrowed_extents: out too small"); return CAFE_ERR_ARGUMENT; }
    if (const int rc = wait_last_call(ctx)) return rc;
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_narrow[node] + (size_t)category * nt * 2, sizeof(int32_t) * 2 * nt, hipMemcpyDeviceToHost));
    return CAFE_OK;
}

// The magnitude tables of the last call's matrices (mag_tables_kernel), one slot's, as the kernel wrote them (units of 1/256,
// kMagNone where every entry is zero): which 0 = a16 [k-steps][16-row blocks], 1 = t4 [k-steps][row steps] (k-major slots),
// 2 = lt [counts 0 .. M][row steps] (row-major slots).  slot < 0: the slot of the branch above `node` in `category`.
int cafe_debug_magnitude_tables(cafe_ctx* ctx, int32_t which, int32_t slot, int32_t* out, size_t out_len, int32_t* n0, int32_t* n1,
                                int32_t node, int32_t category) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_debug_magnitude_tables")) return rc;
    if (which < 0 || which > 2) { set_err(ctx, "cafe_debug_magnitude_tables: which must be 0 (a16), 1 (t4) or 2 (lt)"); return CAFE_ERR_ARGUMENT; }
    if (!ctx->last.magskip || !ctx->d_mag_a16 || !ctx->d_mag_t4 || !ctx->d_mag_lt) {
        set_err(ctx, "cafe_debug_magnitude_tables: the last call kept no tables");
        return CAFE_ERR_STATE;
    }
    const bool leaf_table = which == 2;
    if (slot < 0) {
        if (node < 0 || node >= ctx->n_nodes || node == ctx->root || category < 0 || category >= ctx->last.K ||
            (ctx->leaf_taxon[node] >= 0) != leaf_table) {
            set_err(ctx, "cafe_debug_magnitude_tables: node/category out of range for this table");
            return CAFE_ERR_ARGUMENT;
        }
        slot = ctx->slot_of[(size_t)node * ctx->Kmax + category];
    }
    if (slot < 0 || slot >= (leaf_table ? ctx->last.n_slots : ctx->last.n_kslots)) { set_err(ctx, "cafe_debug_magnitude_tables: slot out of range"); return CAFE_ERR_ARGUMENT; }
    const int d0 = leaf_table ? ctx->M + 1 : ctx->n_ksteps, d1 = which == 0 ? ctx->kpool.ext_blocks : ctx->n_rsteps;
    if (n0) *n0 = d0;
    if (n1) *n1 = d1;
    if (!out) return CAFE_OK;
    if (out_len < (size_t)d0 * d1) { set_err(ctx, "cafe_debug_magnitude_tables: out too small"); return CAFE_ERR_ARGUMENT; }
    if (const int rc = wait_last_call(ctx)) return rc;
    const int32_t* src = which == 0 ? ctx->d_mag_a16 : which == 1 ? ctx->d_mag_t4 : ctx->d_mag_lt;
    HIP_TRY(ctx, hipMemcpy(out, src + (size_t)slot * d0 * d1, sizeof(int32_t) * (size_t)d0 * d1, hipMemcpyDeviceToHost));
    return CAFE_OK;
}

// The joint K ranges of the K2 op that multiplies the matrix of the branch above `node` (an interior non-root node):
// out[(tile * blocks + b) * 2 + {0, 1}] = first / last k-step (4 deep) of 16-row block b against column tile `tile` of the
// node's panel, first > last: none.  *n_tiles = 1 where the panels have no extents (one range per block).
int cafe_debug_k_ranges(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* out, size_t out_len, int32_t* n_tiles, int32_t* n_blocks) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_debug_k_ranges")) return rc;
    if (category < 0 || category >= ctx->last.K) { set_err(ctx, "cafe_debug_k_ranges: category out of range"); return CAFE_ERR_ARGUMENT; }
    const GemmOp* g = nullptr;
    for (const Op& op : ctx->ops) if (op.type == 1 && op.child == node) g = &ctx->h_gemm_ops[op.desc];
    if (!g || !g->jr) { set_err(ctx, "cafe_debug_k_ranges: no K2 op with ranges for this node"); return CAFE_ERR_STATE; }
    const int nb = ctx->kpool.ext_blocks;
    if (n_tiles) *n_tiles = g->jr_nct;
    if (n_blocks) *n_blocks = nb;
    if (!out) return CAFE_OK;
    if (out_len < (size_t)2 * g->jr_nct * nb) { set_err(ctx, "cafe_debug_k_ranges: out too small"); return CAFE_ERR_ARGUMENT; }
    if (const int rc = wait_last_call(ctx)) return rc;
    std::vector<int32_t> jr;
    if (!read_ranges(ctx, *g, ctx->last.K, jr)) { set_err(ctx, "cafe_debug_k_ranges: reading the ranges back failed"); return CAFE_ERR_DEVICE; }
    for (int t = 0; t < g->jr_nct; ++t)
        for (int b = 0; b < nb; ++b) {
            const int32_t v = jr[((size_t)category * g->jr_nct + t) * (nb + kRangePad) + b];
            out[((size_t)t * nb + b) * 2] = v & 0xFFFF; out[((size_t)t * nb + b) * 2 + 1] = v >> 16;
        }
    return CAFE_OK;
}

// The gate of the read-backs that count over the last call's launch list: a completed call, enqueued launch by launch, finished
static int require_launch_list(cafe_ctx* ctx, const char* entry) {
    if (const int rc = require_last(ctx, entry)) return rc;
    if (ctx->gemm_launches_info.empty()) { set_err(ctx, "%s: the last call was not enqueued launch by launch (a graph replay keeps no launch list)", entry); return CAFE_ERR_STATE; }
    return wait_last_call(ctx);
}

static int counted_flops(cafe_ctx* ctx, const char* entry, bool per_block, bool exact, double* flops) {
    if (!ctx || !flops) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_launch_list(ctx, entry)) return rc;
    const double v = count_executed_flops(ctx, nullptr, per_block, exact);
    if (v < 0) { set_err(ctx, "%s: reading the ranges back failed", entry); return CAFE_ERR_DEVICE; }
    *flops = v;
    return CAFE_OK;
}
int cafe_debug_tile_range_flops(cafe_ctx* ctx, double* flops) { return counted_flops(ctx, "cafe_debug_tile_range_flops", false, false, flops); }
int cafe_executed_flops(cafe_ctx* ctx, double* flops) { return counted_flops(ctx, "cafe_executed_flops", true, true, flops); }
int cafe_issued_flops(cafe_ctx* ctx, double* flops) { return counted_flops(ctx, "cafe_issued_flops", true, false, flops); }

// diagnostic / test: read the tile lists of the last call back and check them against the extents -- every tile of every
// op of every launch exactly once, with the K range the extents give, nothing behind the end of a list.
// *n_planned: K2 launches checked; *worst_load: largest planned workgroup load over the mean load of its XCD.
int cafe_debug_plan_check(cafe_ctx* ctx, int32_t* n_planned, double* worst_load) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (n_planned) *n_planned = 0;
    if (worst_load) *worst_load = 1.0;
    const DescSet* ds = ctx->last.desc;
    if (!ds || ctx->last.plan_launches == 0 || ds->plan_desc_sent.empty()) return CAFE_OK;
    if (const int rc = wait_last_call(ctx)) return rc;
    const int jr_row = ctx->kpool.ext_blocks + kRangePad;
    std::vector<int2> plan;
    double worst = 1.0;
    for (const PlanLaunch& L : ds->plan_desc_sent) {
        const int nlb = L.blocks_per_xcd;
        plan.resize((size_t)8 * nlb * L.rounds);
        HIP_TRY(ctx, hipMemcpy(plan.data(), L.plan, plan.size() * sizeof(int2), hipMemcpyDeviceToHost));
        const GemmOp* ops = ds->gemm_ops_sent.data() + (L.ops - ds->d_gemm_ops);
        std::vector<std::vector<int32_t>> op_bext(L.n_ops), op_jr(L.n_ops);
        for (int o = 0; o < L.n_ops; ++o) {
            const int nct = L.uniform_ld > 0 ? L.uniform_ld / kBN : ops[o].n_col_tiles;
            if (ctx->kpool.ext && !read_ranges(ctx, ops[o], L.n_categories, op_jr[o])) { set_err(ctx, "cafe_debug_plan_check: reading the ranges back failed"); return CAFE_ERR_DEVICE; }
            if (ops[o].bext && ctx->kpool.ext) {
                op_bext[o].resize((size_t)2 * L.n_categories * nct);
                HIP_TRY(ctx, hipMemcpy(op_bext[o].data(), ops[o].bext, op_bext[o].size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            }
        }
        for (int x = 0; x < 8; ++x) {
            std::vector<std::vector<char>> seen(L.n_ops);
            for (int o = 0; o < L.n_ops; ++o) {
                const int nct = L.uniform_ld > 0 ? L.uniform_ld / kBN : ops[o].n_col_tiles;
                seen[o].assign((size_t)((L.n_categories * nct - x + 7) >> 3) * ops[o].n_row_tiles, 0);
            }
            double total = 0, top = 0;
            for (int w = 0; w < nlb; ++w) {
                bool ended = false;
                double load = 0;
                for (int r = 0; r < L.rounds; ++r) {
                    const int2 e = plan[((size_t)x * nlb + w) * L.rounds + r];
                    if (e.y == 0) { ended = true; if (e.x != 0) goto bad; continue; }
                    const int o = e.x >> 24, t = e.x & 0xFFFFFF;
                    if (ended || o < 0 || o >= L.n_ops || t >= (int)seen[o].size() || seen[o][t]) goto bad;
                    seen[o][t] = 1;
                    const int nrt = ops[o].n_row_tiles, nct = L.uniform_ld > 0 ? L.uniform_ld / kBN : ops[o].n_col_tiles;
                    const int row_tile = t % nrt, pair = x + 8 * (t / nrt);
                    const int ct = pair % nct, cat = pair / nct, b0 = row_tile * L.mi;
                    int lo = 0, hi = L.k_valid - 1, zlo = 0;
                    if (ctx->kpool.ext) {
                        const int32_t* a = op_jr[o].data() + ((size_t)cat * ops[o].jr_nct + (ct & ops[o].jr_ct_mask)) * jr_row + b0;
                        int slo, shi;
                        const bool any = tile_k_hull(a, L.mi, &slo, &shi);
                        lo = slo * 4; hi = shi * 4 + 3;
                        if (!op_bext[o].empty()) {
                            const int32_t* be = op_bext[o].data() + ((size_t)cat * nct + ct) * 2;
                            if (be[1] >= be[0]) zlo = be[0];
                        }
                        if (!any) { lo = zlo; hi = zlo; }
                        hi = std::min(hi, L.k_valid - 1);
                    }
                    if ((e.y >> 16) != lo / L.kb || (e.y & 0xFFFF) != hi / L.kb - lo / L.kb + 1) goto bad;
                    load += (e.y & 0xFFFF) + L.fixed;
                }
                total += load;
                top = std::max(top, load);
            }
            for (auto& sv : seen) for (char v : sv) if (!v) goto bad;
            if (total > 0) worst = std::max(worst, top / (total / nlb));
        }
        if (n_planned) *n_planned += 1;
        continue;
    bad:
        set_err(ctx, "cafe_debug_plan_check: the tile lists of a launch do not match its K ranges");
        return CAFE_ERR_STATE;
    }
    if (worst_load) *worst_load = worst;
    return CAFE_OK;
}

int cafe_debug_launch_ms(cafe_ctx* ctx, double* ms, size_t n) {      // diagnostic: HIP-event duration of every K2 launch of the last profiled call
    if (!ctx || !ms) return CAFE_ERR_ARGUMENT;
    if (const int rc = wait_last_call(ctx)) return rc;
    for (size_t i = 0; i < n; ++i) {
        float t = 0;
        ms[i] = (2 * i + 1 < ctx->gemm_ev_used && hipEventElapsedTime(&t, ctx->gemm_ev[2 * i], ctx->gemm_ev[2 * i + 1]) == hipSuccess) ? t : 0.0;
    }
    return CAFE_OK;
}

int cafe_debug_launch_flops(cafe_ctx* ctx, double* executed, double* all_k_tiles, int32_t* tile_height, size_t n) {
    if (!ctx || !executed) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_launch_list(ctx, "cafe_debug_launch_flops")) return rc;
    std::vector<double> v;
    if (count_executed_flops(ctx, &v) < 0) { set_err(ctx, "cafe_debug_launch_flops: reading the extents back failed"); return CAFE_ERR_DEVICE; }
    for (size_t i = 0; i < n && i < v.size(); ++i) {
        const auto& L = ctx->gemm_launches_info[i];
        executed[i] = v[i];
        if (all_k_tiles) {
            all_k_tiles[i] = 0;
            for (int oi : ctx->groups[L.group].ops) {
                const Op& op = ctx->ops[oi];
                all_k_tiles[i] += 2.0 * (op.to_root ? ctx->R : ctx->M) * (ctx->M + 1) * (double)panel_cols(ctx, op.child, L.cols) * L.K;
            }
        }
        if (tile_height) tile_height[i] = L.mi;
    }
    return CAFE_OK;
}

// A matrix of order n out of its k-major slot: Pt[c][s-1] = P[s][c] for s >= 1; row 0 of P is e_0, implicit in the layout, and the
// columns c > M are never materialised (the prune never reads them): reported as 0
static void unpack_kmajor(const double* t, const MatrixPool& p, size_t n, double* out) {
    std::fill(out, out + n * n, 0.0);
    out[0] = 1.0;
    for (size_t s = 1; s < n; ++s)
        for (size_t c = 0; c < n && c < (size_t)p.rows; ++c) out[s * n + c] = t[c * (size_t)p.ld + (s - 1)];
}

int cafe_get_matrix(cafe_ctx* ctx, int32_t node, int32_t category, double* out, size_t out_len) {
    if (!ctx || !out) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_get_matrix")) return rc;
    if (node < 0 || node >= ctx->n_nodes || node == ctx->root || category < 0 || category >= ctx->last.K) {
        set_err(ctx, "cafe_get_matrix: node/category out of range");
        return CAFE_ERR_ARGUMENT;
    }
    const size_t n = (size_t)ctx->N;
    if (out_len < n * n) { set_err(ctx, "cafe_get_matrix: out buffer too small"); return CAFE_ERR_ARGUMENT; }
    if (const int rc = wait_last_call(ctx)) return rc;
    const int slot = ctx->slot_of[(size_t)node * ctx->Kmax + category];
    if (ctx->leaf_taxon[node] >= 0) {
        HIP_TRY(ctx, hipMemcpy2D(out, n * sizeof(double), ctx->pool.base + (int64_t)slot * ctx->pool.stride,
                                 (size_t)ctx->pool.ld * sizeof(double), n * sizeof(double), n, hipMemcpyDeviceToHost));
        return CAFE_OK;
    }
    std::vector<double> tmp((size_t)ctx->kpool.rows * ctx->kpool.ld);       // interior branch: stored k-major
    HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->kpool.base + (int64_t)slot * ctx->kpool.stride, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    unpack_kmajor(tmp.data(), ctx->kpool, n, out);
    return CAFE_OK;
}

int cafe_get_root_likelihoods(cafe_ctx* ctx, int64_t family, int32_t category, double* out, size_t out_len) {
    if (!ctx || !out) return CAFE_ERR_ARGUMENT;
    if (const int rc = require_last(ctx, "cafe_get_root_likelihoods")) return rc;
    if (family < 0 || family >= ctx->F_all || category < 0 || category >= ctx->last.K || out_len < (size_t)ctx->R) {
        set_err(ctx, "cafe_get_root_likelihoods: argument out of range");
        return CAFE_ERR_ARGUMENT;
    }
    const int64_t u = ctx->ref_of[family];
    if (u < ctx->last.chunk_f0 || u >= ctx->last.chunk_f0 + ctx->last.chunk_nf) {
        set_err(ctx, "cafe_get_root_likelihoods: family is not in the last resident chunk");
        return CAFE_ERR_STATE;
    }
    if (const int rc = wait_last_call(ctx)) return rc;
    const int64_t cols = std::min<int64_t>(ctx->chunk_cols, ctx->Fp - ctx->last.chunk_f0);
    const cafe::Panel& RP = ctx->panels[ctx->root_panel];
    const double* src = ctx->d_panels + RP.offset + (int64_t)category * RP.kstride + (u - ctx->last.chunk_f0);
    HIP_TRY(ctx, hipMemcpy2D(out, sizeof(double), src, (size_t)cols * sizeof(double), sizeof(double), (size_t)ctx->R, hipMemcpyDeviceToHost));
    return CAFE_OK;
}

// cafe_build_matrices (mus == nullptr: K1) and cafe_build_matrices_lm (the two-rate kernel)
static int build_matrices(int32_t device, int32_t n, int32_t count, const double* lambdas, const double* mus, const double* ts, int32_t layout, double* out) {
    if (n < 2 || count < 1 || !lambdas || !ts || !out || n > bd_matrix_max_order()) return CAFE_ERR_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return CAFE_ERR_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return CAFE_ERR_DEVICE;
    MatrixPool pool = row_major_pool(n);
    if (layout != 0) {
        pool.rows = round_up(n, kBK); pool.k_valid = n; pool.kmajor = 1;
        pool.ld = round_up(n - 1, 16) + 16; pool.stride = (int64_t)pool.rows * pool.ld;
    }
    std::vector<SlotParam> sp(mus ? 0 : count);
    std::vector<SlotParamLM> sp_lm(mus ? count : 0);
    for (int i = 0; i < count; ++i) {
        if (mus) sp_lm[i] = slot_param_lm(quantize_lambda(lambdas[i]), quantize_lambda(mus[i]), quantize_time(ts[i]));
        else sp[i] = slot_param(quantize_lambda(lambdas[i]), quantize_time(ts[i]));
    }
    const size_t sp_bytes = mus ? sizeof(SlotParamLM) * count : sizeof(SlotParam) * count;
    const void* h_sp = mus ? (const void*)sp_lm.data() : (const void*)sp.data();
    void* d_sp = nullptr;
    int rc = CAFE_OK;
    const size_t bytes = sizeof(double) * pool.stride * count;
    if (hipMalloc(&pool.base, bytes) != hipSuccess) return CAFE_ERR_MEMORY;
    if (hipMalloc(&d_sp, sp_bytes) != hipSuccess) { (void)hipFree(pool.base); return CAFE_ERR_MEMORY; }
    if (hipMemset(pool.base, 0, bytes) != hipSuccess) rc = CAFE_ERR_DEVICE;
    if (rc == CAFE_OK && hipMemcpy(d_sp, h_sp, sp_bytes, hipMemcpyHostToDevice) != hipSuccess) rc = CAFE_ERR_DEVICE;
    if (rc == CAFE_OK && (mus ? launch_bd_matrix_build(pool, static_cast<const SlotParamLM*>(d_sp), count, nullptr)
                              : launch_bd_matrix_build(pool, static_cast<const SlotParam*>(d_sp), count, nullptr)) != hipSuccess)
        rc = CAFE_ERR_DEVICE;
    if (rc == CAFE_OK && hipDeviceSynchronize() != hipSuccess) rc = CAFE_ERR_DEVICE;
    std::vector<double> tmp;
    for (int i = 0; i < count && rc == CAFE_OK; ++i) {
        double* o = out + (size_t)i * n * n;
        if (layout == 0) {
            if (hipMemcpy2D(o, (size_t)n * sizeof(double), pool.base + (int64_t)i * pool.stride, (size_t)pool.ld * sizeof(double),
                            (size_t)n * sizeof(double), n, hipMemcpyDeviceToHost) != hipSuccess)
                rc = CAFE_ERR_DEVICE;
        } else {
            tmp.resize((size_t)pool.stride);
            if (hipMemcpy(tmp.data(), pool.base + (int64_t)i * pool.stride, tmp.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
                rc = CAFE_ERR_DEVICE;
                break;
            }
            unpack_kmajor(tmp.data(), pool, (size_t)n, o);
        }
    }
    (void)hipFree(pool.base);
    (void)hipFree(d_sp);
    return rc;
}

int cafe_build_matrices(int32_t device, int32_t n, int32_t count, const double* lambdas, const double* ts, int32_t layout, double* out) {
    return build_matrices(device, n, count, lambdas, nullptr, ts, layout, out);
}

int cafe_build_matrices_lm(int32_t device, int32_t n, int32_t count, const double* lambdas, const double* mus, const double* ts, int32_t layout, double* out) {
    if (!mus) return CAFE_ERR_ARGUMENT;
    return build_matrices(device, n, count, lambdas, mus, ts, layout, out);
}

int cafe_probe_fp64_mfma(int32_t device, double* tflops) {
    if (!tflops) return CAFE_ERR_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return CAFE_ERR_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return CAFE_ERR_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CAFE_ERR_DEVICE;
    const int blocks = prop.multiProcessorCount * 2, iters = 20000;
    double* d = nullptr;
    if (hipMalloc(&d, sizeof(double) * 256 * blocks) != hipSuccess) return CAFE_ERR_MEMORY;
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    (void)launch_mfma_probe(d, 200, blocks, nullptr);      // warm-up
    (void)hipEventRecord(a, nullptr);
    (void)launch_mfma_probe(d, iters, blocks, nullptr);
    (void)hipEventRecord(b, nullptr);
    int rc = hipEventSynchronize(b) == hipSuccess ? CAFE_OK : CAFE_ERR_DEVICE;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    // each wave issues iters * 8 MFMAs of 16*16*4*2 flops
    const double flops = (double)blocks * 4 /*waves*/ * iters * 8.0 * 2048.0;
    *tflops = ms > 0 ? flops / (ms * 1e-3) / 1e12 : 0.0;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipFree(d);
    return rc;
}

}  // extern "C"
