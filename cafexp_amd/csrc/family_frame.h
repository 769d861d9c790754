// The host frame of the per-family entries (family_lambda.hip has the reasoning): cafe_score_per_family and
// cafe_score_per_family_lm (family_lambda.hip) and cafe_score_per_family_gain (family_gain.hip).  What the entries differ in
// is a Kind:
//   Slot, entry, reads_context_rates     the slot type of the branch kernel, the entry's name, whether lambda = mu is assumed
//   absent_ok                            whether family[i] == CAFE_FAMILY_ABSENT (the all-zero profile, column -1) is accepted
//   rates_ok(L, mus_i, nus_i)            the entry's rule for the rates beside lambdas_valid
//   slot(c, u, lam, mus, nus)            the slot of the branch above node u under one family's rates
//   branches(a, n, batch, nodes, s)      one level of branches
//   root(c, ra, batch, s)                the root kernel of the context's root rule
// mus and nus are [n][n_lambdas] or null, as the entry defines them.
//
// An entry that goes on where the root kernel stops (family_gain_posterior.hip: the down pass) hands the frame a Tail: device
// bytes of its own behind the factors -- counted into the batch size -- one call when the workspace stands, one behind the root
// kernel of every batch, one behind the batch's synchronisation.  The score entries pass FamNoTail: no byte, no call.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "cafe_call.h"
#include "family_lambda_kernel.h"

namespace cafe {

struct FamRootArgs {
    const int32_t* root_children;
    int32_t n_root_children, R, ld, n_nodes;
    const double* log_prior;         // [R] log((double)float prior), host libm
    const double* factors;
    double* out;                     // [batch]
};

// rates_valid's rule for the death rates of one entry (mus[L]; a NaN fails it)
inline bool death_rates_ok(int L, const double* mus) {
    for (int k = 0; mus && k < L; ++k)
        if (!(mus[k] >= 0)) return false;
    return true;
}
// The branch above node u under (lambdas, mus): either rate beyond a long saturates the branch
inline SlotParamLM branch_param_lm(const cafe_ctx* c, int u, const double* lam, const double* mus) {
    const double l = lam[c->lam_idx[u]], m = mus[c->lam_idx[u]];
    if (!(l * 1000000000 < 9.0e18) || !(m * 1000000000 < 9.0e18)) {
        SlotParamLM sp{};
        sp.alpha = 1.0; sp.beta = 1.0; sp.q = 0.0; sp.zero = 1;
        return sp;
    }
    return slot_param_lm(quantize_lambda(l), quantize_lambda(m), quantize_time(c->blen[u]));
}

inline size_t family_align_up(size_t v) { return (v + 255) / 256 * 256; }

struct FamNoTail {
    size_t static_bytes(const cafe_ctx*) const { return 0; }
    size_t family_bytes(const cafe_ctx*, int) const { return 0; }
    template <class Slot>
    int begin(cafe_ctx*, const FamLamArgs<Slot>&, const FamRootArgs&, char*, char*, int64_t, hipStream_t) { return CAFE_OK; }
    int run(cafe_ctx*, int64_t, hipStream_t) { return CAFE_OK; }
    void collect(const int64_t*, const double*, int64_t) {}
};

// The host frame of every entry: argument checks, what the host decides alone, levels and tables, the batches under the
// workspace limit, one launch per level and the root kernel.
template <class Kind, class Tail>
int per_family_frame(const Kind& kind, Tail& tail, cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas,
                     const double* mus, const double* nus, double* family_lnl) {
    using Slot = typename Kind::Slot;
    const char* const who = Kind::entry;
    if (!pr || !pr->prior) { set_err(c, "%s: params with a prior are required", who); return CAFE_ERR_ARGUMENT; }
    if (pr->model != CAFE_MODEL_BASE) { set_err(c, "%s: base model only", who); return CAFE_ERR_ARGUMENT; }
    if (c->comm) { set_err(c, "%s: not valid on a context with a communicator attached", who); return CAFE_ERR_STATE; }
    if (Kind::reads_context_rates && !c->mus.empty()) { set_err(c, "%s: not valid while death rates are set (cafe_set_death_rates)", who); return CAFE_ERR_STATE; }
    if (n < 0 || (n > 0 && (!family || !lambdas || !family_lnl))) { set_err(c, "%s: family, lambdas and family_lnl are required", who); return CAFE_ERR_ARGUMENT; }
    if ((c->n_dev > 0) != (pr->error_model != nullptr)) {
        set_err(c, "%s: error model %s but the problem was created with n_deviations=%d", who, pr->error_model ? "given" : "missing", c->n_dev);
        return CAFE_ERR_ARGUMENT;
    }
    if (!c->device_ready || !c->d_counts) { set_err(c, "%s: the context holds no family table", who); return CAFE_ERR_STATE; }
    for (int64_t i = 0; i < n; ++i)
        if ((family[i] < 0 && !(Kind::absent_ok && family[i] == -1)) || family[i] >= c->F_all) {
            set_err(c, "%s: family index %lld outside 0..%lld", who, (long long)family[i], (long long)c->F_all - 1);
            return CAFE_ERR_ARGUMENT;
        }
    if (n == 0) return CAFE_OK;
    const int nn = c->n_nodes, L = c->n_lambdas, ld = round_up(c->N, 2);

    // ---- what the host decides alone: an invalid vector is -inf (base_model.cpp:56-60); a NaN that passes is_valid stays NaN
    std::vector<int64_t> active;
    active.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double* lam = lambdas + i * L;
        bool nan = false, valid = lambdas_valid(c, lam);
        for (int k = 0; k < L; ++k) nan = nan || std::isnan(lam[k]);
        valid = valid && Kind::rates_ok(L, mus ? mus + i * L : nullptr, nus ? nus + i * L : nullptr);
        if (!valid) family_lnl[i] = -std::numeric_limits<double>::infinity();
        else if (nan) family_lnl[i] = std::numeric_limits<double>::quiet_NaN();
        else active.push_back(i);
    }
    c->last.state = LastCall::kNone;                   // cafe_family_results is not meaningful after this call
    if (active.empty()) return CAFE_OK;
    const int64_t na = (int64_t)active.size();

    // ---- static tables: children lists, levels (a branch is ready when the factors of the node's children are)
    std::vector<int32_t> child_off(nn + 1, 0), child_idx, level(nn, 0), n_rows(nn, 0), level_nodes, root_children;
    std::vector<int> level_off{0};
    int n_levels = 0;
    for (int u = 0; u < nn; ++u) {
        child_off[u] = (int32_t)child_idx.size();
        for (int ch : c->children[u]) { child_idx.push_back(ch); level[u] = std::max(level[u], level[ch] + 1); }
        if (u != c->root) { n_rows[u] = (c->parent[u] == c->root ? c->R : c->M) + 1; n_levels = std::max(n_levels, level[u] + 1); }
    }
    child_off[nn] = (int32_t)child_idx.size();
    for (int lv = 0; lv < n_levels; ++lv) {
        for (int u = 0; u < nn; ++u) if (u != c->root && level[u] == lv) level_nodes.push_back(u);
        level_off.push_back((int)level_nodes.size());
    }
    for (int ch : c->children[c->root]) root_children.push_back(ch);
    std::vector<int32_t> tables;                       // child_off, child_idx, taxon, n_rows, level_nodes, root_children
    const size_t o_child_idx = (size_t)nn + 1, o_taxon = o_child_idx + child_idx.size(), o_rows = o_taxon + nn, o_level = o_rows + nn,
                 o_rootch = o_level + level_nodes.size();
    tables.insert(tables.end(), child_off.begin(), child_off.end());
    tables.insert(tables.end(), child_idx.begin(), child_idx.end());
    tables.insert(tables.end(), c->leaf_taxon.begin(), c->leaf_taxon.end());
    tables.insert(tables.end(), n_rows.begin(), n_rows.end());
    tables.insert(tables.end(), level_nodes.begin(), level_nodes.end());
    tables.insert(tables.end(), root_children.begin(), root_children.end());
    std::vector<double> reals((size_t)c->R + (size_t)(c->M + 1) * c->n_dev);      // log prior, error model
    for (int j = 0; j < c->R; ++j) reals[j] = std::log((double)pr->prior[j]);    // compute() returns float (root_equilibrium_distribution.h:15)
    if (c->n_dev > 0) std::memcpy(reals.data() + c->R, pr->error_model, sizeof(double) * (size_t)(c->M + 1) * c->n_dev);

    // ---- the batch: as many listed families as the workspace holds
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t tail_static = family_align_up(tail.static_bytes(c)), tail_family = tail.family_bytes(c, ld), tail_pad = tail_static + tail_family ? 256 : 0;
    const size_t static_bytes = family_align_up(sizeof(int32_t) * tables.size()) + family_align_up(sizeof(double) * reals.size()) + tail_static + tail_pad;
    const size_t family_bytes = sizeof(double) * (size_t)nn * ld + sizeof(Slot) * (size_t)nn + sizeof(int64_t) + sizeof(double) + tail_family;
    size_t budget = 0;
    HIP_TRY(c, workspace_budget(c->workspace_limit, c->pf_dev_bytes, &budget));
    int64_t batch = std::max<int64_t>(1, std::min<int64_t>(na, budget > static_bytes + 1024 ? (int64_t)((budget - static_bytes - 1024) / family_bytes) : 1));
    if (c->pf_max_batch > 0) batch = std::min(batch, c->pf_max_batch);
    const size_t o_reals = family_align_up(sizeof(int32_t) * tables.size()), o_col = o_reals + family_align_up(sizeof(double) * reals.size()),
                 o_out = o_col + family_align_up(sizeof(int64_t) * batch), o_slots = o_out + family_align_up(sizeof(double) * batch),
                 o_fac = o_slots + family_align_up(sizeof(Slot) * (size_t)batch * nn), fac_end = o_fac + sizeof(double) * (size_t)batch * nn * ld,
                 o_tail = tail_pad ? family_align_up(fac_end) : fac_end, need = o_tail + tail_static + tail_family * (size_t)batch;
    if (need > c->pf_dev_bytes) {
        if (c->pf_dev) { HIP_TRY(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->pf_dev); c->pf_dev = nullptr; c->pf_dev_bytes = 0; }
        if (hipMalloc(&c->pf_dev, need) != hipSuccess) {
            (void)hipGetLastError();
            c->pf_dev = nullptr;
            set_err(c, "%s: cannot allocate a workspace of %zu bytes (%lld families per batch)", who, need, (long long)batch);
            return CAFE_ERR_MEMORY;
        }
        c->pf_dev_bytes = need;
    }
    char* base = static_cast<char*>(c->pf_dev);
    const int32_t* d_tables = reinterpret_cast<const int32_t*>(base);
    const double* d_reals = reinterpret_cast<const double*>(base + o_reals);
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(base, tables.data(), sizeof(int32_t) * tables.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(base + o_reals, reals.data(), sizeof(double) * reals.size(), hipMemcpyHostToDevice, s));

    FamLamArgs<Slot> a{};
    a.child_off = d_tables; a.child_idx = d_tables + o_child_idx; a.taxon = d_tables + o_taxon; a.n_rows = d_tables + o_rows;
    a.slots = reinterpret_cast<const Slot*>(base + o_slots);
    a.col = reinterpret_cast<const int64_t*>(base + o_col);
    a.counts = c->d_counts; a.counts_ld = c->Fp;
    a.err = c->n_dev > 0 ? d_reals + c->R : nullptr;
    a.n_dev = c->n_dev; a.M = c->M; a.ld = ld; a.n_nodes = nn;
    a.factors = reinterpret_cast<double*>(base + o_fac);
    FamRootArgs ra{};
    ra.root_children = d_tables + o_rootch; ra.n_root_children = (int32_t)root_children.size();
    ra.R = c->R; ra.ld = ld; ra.n_nodes = nn; ra.log_prior = d_reals; ra.factors = a.factors;
    ra.out = reinterpret_cast<double*>(base + o_out);
    if (const int rc = tail.begin(c, a, ra, base + o_tail, base + o_tail + tail_static, batch, s)) return rc;

    std::vector<Slot> slots((size_t)batch * nn);
    std::vector<int64_t> col((size_t)batch);
    std::vector<double> res((size_t)batch);
    for (int64_t b0 = 0; b0 < na; b0 += batch) {
        const int64_t nb = std::min(batch, na - b0);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t i = active[b0 + b];
            col[b] = family[i] < 0 ? -1 : c->ref_of[family[i]];
            for (int u = 0; u < nn; ++u)
                slots[(size_t)b * nn + u] = u == c->root ? Slot{} : Kind::slot(c, u, lambdas + i * L, mus ? mus + i * L : nullptr, nus ? nus + i * L : nullptr);
        }
        HIP_TRY(c, hipMemcpyAsync(base + o_slots, slots.data(), sizeof(Slot) * (size_t)nb * nn, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(base + o_col, col.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
        for (int lv = 0; lv < n_levels; ++lv) {
            a.nodes = d_tables + o_level + level_off[lv];
            HIP_TRY(c, Kind::branches(a, c->N, nb, level_off[lv + 1] - level_off[lv], s));
        }
        HIP_TRY(c, kind.root(c, ra, nb, s));
        if (const int rc = tail.run(c, nb, s)) return rc;
        HIP_TRY(c, hipMemcpyAsync(res.data(), base + o_out, sizeof(double) * nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));            // the host tables of this batch go out of use
        for (int64_t b = 0; b < nb; ++b) family_lnl[active[b0 + b]] = res[b];
        tail.collect(active.data() + b0, res.data(), nb);
    }
    return CAFE_OK;
}

template <class Kind>
int per_family_frame(const Kind& kind, cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                     const double* nus, double* family_lnl) {
    FamNoTail none;
    return per_family_frame(kind, none, c, pr, n, family, lambdas, mus, nus, family_lnl);
}

// What family_gain.hip lends the entries that run its kernels (family_gain_posterior.hip): the checks of nus and root_absent, the
// slot of a branch and the sum-rule root kernel whatever the context's root rule is.
struct SlotParamGain;
int gain_rates_check(cafe_ctx* c, const char* who, int64_t n, const double* nus, double root_absent);
SlotParamGain gain_branch_slot(const cafe_ctx* c, int u, const double* lam, const double* mus, const double* nus);
hipError_t gain_root_sum(const FamRootArgs& ra, double root_absent, int64_t nb, hipStream_t s);

}  // namespace cafe
