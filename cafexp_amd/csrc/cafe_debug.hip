// Diagnostics and read-backs of the C ABI: what the last call built and ran (matrices, extents, tile lists, executed
// flops, launch times), the test hooks, and the two context-free probes.  Nothing here is on the scorer path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cafe_call.h"

using namespace cafe;

namespace cafe {

// Flops the K2 launches of the last (profiled) call EXECUTED: a (row tile, column tile) pair runs only the K tiles inside
// matrix extent x panel extent, so read the extents this call published and count, per launch, what its tiles ran.  Reads
// the extents back (a few synchronous copies, milliseconds of host work): for measurement, once, not per call.
// per_block: count a row block only over the k-steps (4 deep) inside its own extent and the panel's (what the kernel issues,
// prune_gemm.hip block_ranges); false: every block over its tile's whole K range (the count of rounds 2 and 3a, kept for
// comparison).  Both count the valid k and rows only (a ragged last k-step counts its k <= M, a ragged last block its rows).
double count_executed_flops(cafe_ctx* c, std::vector<double>* per_launch, bool per_block) {
    if (c->gemm_launches_info.empty()) return c->stats.gemm_flops;
    const int kBK = c->kb;
    const int nb = c->kpool.ext_blocks;
    std::vector<int32_t> ext;
    if (c->kpool.ext) {
        ext.resize((size_t)2 * c->max_kslots * nb);
        if (hipMemcpy(ext.data(), c->kpool.ext, ext.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
    }
    double executed = 0;
    std::vector<int32_t> bext;
    for (const auto& L : c->gemm_launches_info) {
        const double before = executed;
        const int mi = L.mi, bm = 16 * mi;
        for (int oi : c->groups[L.group].ops) {
            const Op& op = c->ops[oi];
            const int rows = op.to_root ? c->R : c->M;
            const int64_t cols = panel_cols(c, op.child, L.cols);
            const int n_ct = (int)(cols / kBN);
            const bool have_b = c->kpool.ext && c->panel_extents && c->d_tileext[op.child];
            if (have_b) {
                bext.resize((size_t)2 * L.K * n_ct);
                if (hipMemcpy(bext.data(), c->d_tileext[op.child], bext.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
            }
            for (int k = 0; k < L.K; ++k) {
                const int32_t* e = c->kpool.ext ? ext.data() + (size_t)c->slot_of[(size_t)op.child * c->Kmax + k] * nb * 2 : nullptr;
                for (int row0 = 0; row0 < rows; row0 += bm) {
                    int alo = 0, ahi = c->M;
                    if (e) {
                        alo = 0x7fffffff; ahi = -1;
                        for (int b = row0 / 16; b < row0 / 16 + mi && b < nb; ++b) { alo = std::min(alo, e[2 * b]); ahi = std::max(ahi, e[2 * b + 1]); }
                    }
                    for (int ct = 0; ct < (have_b ? n_ct : 1); ++ct) {
                        int lo = alo, hi = ahi, plo = 0, phi = c->M;
                        if (have_b) {
                            plo = bext[((size_t)k * n_ct + ct) * 2]; phi = std::min(c->M, bext[((size_t)k * n_ct + ct) * 2 + 1]);
                            lo = std::max(lo, plo); hi = std::min(hi, phi);
                            if (bext[((size_t)k * n_ct + ct) * 2 + 1] < plo) { plo = 0; phi = 0; }      // an empty panel extent: row 0 (extents.hip)
                        }
                        if (hi < lo) { lo = 0; hi = 0; }
                        hi = std::min(hi, c->M);
                        // the tile runs K tiles lo/kb .. hi/kb; its row block b issues MFMAs only in the k-steps that meet ITS OWN
                        // extent cut by the panel's (prune_gemm.hip, block_ranges); the last k-step of the matrix is ragged
                        const int t_lo = lo / kBK, t_hi = hi / kBK;
                        for (int b = row0 / 16; b < row0 / 16 + mi && b * 16 < rows; ++b) {
                            int kk;
                            if (e && per_block) {
                                if (b >= nb) continue;
                                const int s_lo = std::max(e[2 * b], plo), s_hi = std::min(e[2 * b + 1], phi);
                                if (s_hi < s_lo) continue;
                                kk = std::min((s_hi / 4 - s_lo / 4 + 1) * 4, c->M + 1 - s_lo / 4 * 4);
                            } else {
                                kk = std::min((t_hi - t_lo + 1) * kBK, c->M + 1 - t_lo * kBK);
                            }
                            executed += 2.0 * std::min(16, rows - b * 16) * (double)kk * (have_b ? (double)kBN : (double)cols);
                        }
                    }
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

int cafe_get_extents(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* matrix_ext, size_t matrix_ext_len,
                     int32_t* panel_ext, size_t panel_ext_len, int32_t* n_tiles) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (!ctx->have_results || ctx->last_rejected) { set_err(ctx, "cafe_get_extents: no completed call"); return CAFE_ERR_STATE; }
    if (node < 0 || node >= ctx->n_nodes || node == ctx->root || category < 0 || category >= ctx->K_last) {
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
    if (used_by_last_call) *used_by_last_call = ctx->lt_used_last ? 1 : 0;
    return CAFE_OK;
}

int cafe_debug_column_extents(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* out, size_t out_len, int64_t* n_cols) {
    if (!ctx || !out) return CAFE_ERR_ARGUMENT;
    if (!ctx->have_results || ctx->last_rejected) { set_err(ctx, "cafe_debug_column_extents: no completed call"); return CAFE_ERR_STATE; }
    if (node < 0 || node >= ctx->n_nodes || category < 0 || category >= ctx->K_last || !ctx->panel_extents || !ctx->d_colext[node]) {
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

int cafe_debug_tile_range_flops(cafe_ctx* ctx, double* flops) {
    if (!ctx || !flops) return CAFE_ERR_ARGUMENT;
    if (!ctx->have_results || ctx->gemm_launches_info.empty()) { set_err(ctx, "cafe_debug_tile_range_flops: no completed call that was enqueued launch by launch"); return CAFE_ERR_STATE; }
    if (const int rc = wait_last_call(ctx)) return rc;
    const double v = count_executed_flops(ctx, nullptr, false);
    if (v < 0) { set_err(ctx, "cafe_debug_tile_range_flops: reading the extents back failed"); return CAFE_ERR_DEVICE; }
    *flops = v;
    return CAFE_OK;
}

int cafe_executed_flops(cafe_ctx* ctx, double* flops) {
    if (!ctx || !flops) return CAFE_ERR_ARGUMENT;
    if (!ctx->have_results) { set_err(ctx, "cafe_executed_flops: no completed call"); return CAFE_ERR_STATE; }
    if (const int rc = wait_last_call(ctx)) return rc;
    if (ctx->gemm_launches_info.empty()) { set_err(ctx, "cafe_executed_flops: the last call was not enqueued launch by launch (a graph replay keeps no launch list)"); return CAFE_ERR_STATE; }
    const double v = count_executed_flops(ctx);
    if (v < 0) { set_err(ctx, "cafe_executed_flops: reading the extents back failed"); return CAFE_ERR_DEVICE; }
    *flops = v;
    return CAFE_OK;
}

// diagnostic / test: read the tile lists of the last call back and check them against the extents -- every tile of every
// op of every launch exactly once, with the K range the extents give, nothing behind the end of a list.
// *n_planned: K2 launches checked; *worst_load: largest planned workgroup load over the mean load of its XCD.
int cafe_debug_plan_check(cafe_ctx* ctx, int32_t* n_planned, double* worst_load) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (n_planned) *n_planned = 0;
    if (worst_load) *worst_load = 1.0;
    const DescSet* ds = ctx->desc_last;
    if (!ds || ctx->plan_launches_last == 0 || ds->plan_desc_sent.empty()) return CAFE_OK;
    if (const int rc = wait_last_call(ctx)) return rc;
    const int nb = ctx->kpool.ext_blocks;
    std::vector<int32_t> aext, bext;
    if (ctx->kpool.ext) {
        aext.resize((size_t)2 * ctx->max_kslots * nb);
        HIP_TRY(ctx, hipMemcpy(aext.data(), ctx->kpool.ext, aext.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    std::vector<int2> plan;
    double worst = 1.0;
    for (const PlanLaunch& L : ds->plan_desc_sent) {
        const int nlb = L.blocks_per_xcd;
        plan.resize((size_t)8 * nlb * L.rounds);
        HIP_TRY(ctx, hipMemcpy(plan.data(), L.plan, plan.size() * sizeof(int2), hipMemcpyDeviceToHost));
        const GemmOp* ops = ds->gemm_ops_sent.data() + (L.ops - ds->d_gemm_ops);
        std::vector<std::vector<int32_t>> op_bext(L.n_ops);
        for (int o = 0; o < L.n_ops; ++o) {
            const int nct = L.uniform_ld > 0 ? L.uniform_ld / kBN : ops[o].n_col_tiles;
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
                        const int32_t* a = aext.data() + ((size_t)ops[o].slot[cat] * nb + b0) * 2;
                        lo = 0x7fffffff; hi = -1;
                        for (int b = 0; b < L.mi && b0 + b < nb; ++b) { lo = std::min(lo, a[2 * b]); hi = std::max(hi, a[2 * b + 1]); }
                        if (!op_bext[o].empty()) {
                            const int32_t* be = op_bext[o].data() + ((size_t)cat * nct + ct) * 2;
                            lo = std::max(lo, be[0]); hi = std::min(hi, be[1]);
                            if (be[1] >= be[0]) zlo = be[0];
                        }
                        if (hi < lo) { lo = zlo; hi = zlo; }
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
        set_err(ctx, "cafe_debug_plan_check: the tile lists of a launch do not match its extents");
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
    if (!ctx->have_results || ctx->gemm_launches_info.empty()) { set_err(ctx, "cafe_debug_launch_flops: no call enqueued launch by launch"); return CAFE_ERR_STATE; }
    if (const int rc = wait_last_call(ctx)) return rc;
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
    return (int)std::min(n, v.size()) >= 0 ? CAFE_OK : CAFE_OK;
}

int cafe_get_matrix(cafe_ctx* ctx, int32_t node, int32_t category, double* out, size_t out_len) {
    if (!ctx || !out) return CAFE_ERR_ARGUMENT;
    if (!ctx->have_results) { set_err(ctx, "cafe_get_matrix: no completed call"); return CAFE_ERR_STATE; }
    if (node < 0 || node >= ctx->n_nodes || node == ctx->root || category < 0 || category >= ctx->K_last) {
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
    // interior branch: stored k-major, Pt[c][s-1] = P[s][c] for c <= M, s >= 1; row 0 of P is e_0 and the
    // columns c > M are never materialised (the prune never reads them): reported as 0
    const size_t ldt = (size_t)ctx->kpool.ld, rows = (size_t)ctx->kpool.rows;
    std::vector<double> tmp(rows * ldt);
    HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->kpool.base + (int64_t)slot * ctx->kpool.stride, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::fill(out, out + n * n, 0.0);
    out[0] = 1.0;
    for (size_t s2 = 1; s2 < n; ++s2)
        for (size_t c2 = 0; c2 < n && c2 < rows; ++c2) out[s2 * n + c2] = tmp[c2 * ldt + (s2 - 1)];
    return CAFE_OK;
}

int cafe_get_root_likelihoods(cafe_ctx* ctx, int64_t family, int32_t category, double* out, size_t out_len) {
    if (!ctx || !out) return CAFE_ERR_ARGUMENT;
    if (!ctx->have_results || ctx->last_rejected) { set_err(ctx, "cafe_get_root_likelihoods: no completed call"); return CAFE_ERR_STATE; }
    if (family < 0 || family >= ctx->F_all || category < 0 || category >= ctx->K_last || out_len < (size_t)ctx->R) {
        set_err(ctx, "cafe_get_root_likelihoods: argument out of range");
        return CAFE_ERR_ARGUMENT;
    }
    const int64_t u = ctx->ref_of[family];
    if (u < ctx->last_chunk_f0 || u >= ctx->last_chunk_f0 + ctx->last_chunk_nf) {
        set_err(ctx, "cafe_get_root_likelihoods: family is not in the last resident chunk");
        return CAFE_ERR_STATE;
    }
    if (const int rc = wait_last_call(ctx)) return rc;
    const int64_t cols = std::min<int64_t>(ctx->chunk_cols, ctx->Fp - ctx->last_chunk_f0);
    const cafe::Panel& RP = ctx->panels[ctx->root_panel];
    const double* src = ctx->d_panels + RP.offset + (int64_t)category * RP.kstride + (u - ctx->last_chunk_f0);
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
            std::fill(o, o + (size_t)n * n, 0.0);
            o[0] = 1.0;                                    // P's row 0 = e_0 is implicit in the k-major layout
            for (int s2 = 1; s2 < n; ++s2)
                for (int c2 = 0; c2 < n; ++c2) o[(size_t)s2 * n + c2] = tmp[(size_t)c2 * pool.ld + (s2 - 1)];
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
