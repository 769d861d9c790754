// cafe_score_per_family: one scorer evaluation for a list of families, EACH WITH ITS OWN lambdas -- what the reference's
// lambda-per-family mode (-b; estimator::estimate_lambda_per_family, src/execute.cpp:104-128) asks of the scorer, one
// family at a time.
//
// With one lambda vector per family nothing of the scorer path applies: every family has its own transition matrices, a
// branch is a matrix-vector product and not a GEMM, and a matrix is used exactly once.  So no matrix is ever written:
//   branch kernel   ONE 64-lane wave per (listed family, branch).  The wave loads the child's likelihood vector v (a leaf:
//                   one-hot at the observed count, or the error-model taps around it; an interior node: the product of its
//                   children's factors, multiplied on load), runs K1's row recurrence (bd_row.h: a lane owns E consecutive
//                   columns of the row, DPP scan; the same quantized key, the same special cases) and after every row step
//                   forms factor[s] = sum_c P[s][c] v[c], c = 0..M.
//   the dot product The lane partials of a row must be summed across the wave, and that sum must not sit on the dependent
//                   chain of row steps (a row step IS the kernel's latency).  A lane parks its partial in LDS
//                   (part[row % 16][lane]) and goes on; every 16 rows the block is summed transposed -- lane (j, quarter)
//                   adds 16 partials of row j, two cross-lane adds fold the quarters -- and 16 lanes store 16 factors.
//                   16 rows and not 64: 8 KB of LDS per wave instead of 33 KB, so LDS never limits the waves per CU.
//   levels          Children first, ONE LAUNCH PER LEVEL over (families x branches of the level): the unit of work stays
//                   one wave whatever the tree's shape, a launch of the mammals table has >= 12 653 waves, and late in a
//                   search -- few unfinished families -- the branches of a level still spread over the chip, which one
//                   workgroup per family (a barrier per level, as many waves as the widest level) would not.
//   root kernel     one wave per family: L[j] = prod_children factor[j + 1], j = 0..R-1, then what K4 applies:
//                   max_j(log L_j + log (double)(float)prior_j) (base_model.cpp:95-102).
// Factors live in a workspace [listed family][node][ld] doubles.  The list is cut into batches that fit the context's
// workspace_limit (0 = automatic); a family's value depends on its counts and lambdas only, never on the cut.
// Every leaf branch runs all its rows (the reversibility short cut for a leaf without error model -- c row steps for a
// count c -- is not taken).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "cafe_call.h"
#include "family_lambda_kernel.h"

namespace cafe {

// the branch kernel (family_lambda_kernel.h) for lambda = mu; family_lambda_lm.hip holds the two-rate instantiation
template hipError_t launch_family_lambda<SlotParam>(const FamLamArgs<SlotParam>&, int, int64_t, int, hipStream_t);

namespace {

struct FamRootArgs {
    const int32_t* root_children;
    int32_t n_root_children, R, ld, n_nodes;
    const double* log_prior;         // [R] log((double)float prior), host libm
    const double* factors;
    double* out;                     // [batch]
};

// lnL_f = max_j(log L_j + log prior_j) (base_model.cpp:94-101), L_j = prod over the root's children of factor[j + 1]
__global__ __launch_bounds__(64) void family_root_kernel(const FamRootArgs a) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* __restrict__ fac_b = a.factors + b * a.n_nodes * a.ld;
    double best = -__builtin_huge_val();
    for (int j = lane; j < a.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.n_root_children; ++k) L *= fac_b[(int64_t)a.root_children[k] * a.ld + j + 1];
        const double full = log(L) + a.log_prior[j];
        if (j == 0 || full > best) best = full;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_down(best, d);
        if (o > best) best = o;
    }
    if (lane == 0) a.out[b] = best;
}

// ... and under CAFE_ROOT_SUM (cafe_set_root_rule) lnL_f = log sum_j L_j prior_j as K4's sum rule evaluates it: m = max_j t_j,
// t_j = log L_j + log prior_j, then m + log sum_j exp(t_j - m) -- a lane adds its rows j = lane, lane + 64, ... in ascending
// order, the lanes are folded by a fixed tree.  All t_j = -inf: -inf; a NaN term: NaN.  A kernel of its own: the max rule's
// code stays what it was.
__global__ __launch_bounds__(64) void family_root_sum_kernel(const FamRootArgs a) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double* __restrict__ fac_b = a.factors + b * a.n_nodes * a.ld;
    const double ninf = -__builtin_huge_val();
    double m = ninf;
    for (int j = lane; j < a.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.n_root_children; ++k) L *= fac_b[(int64_t)a.root_children[k] * a.ld + j + 1];
        const double t = log(L) + a.log_prior[j];
        if (t > m) m = t;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                // (butterfly: every lane ends with the maximum)
        const double o = __shfl_xor(m, d);
        if (o > m) m = o;
    }
    double s = 0.0;
    for (int j = lane; j < a.R; j += 64) {
        double L = 1.0;
        for (int k = 0; k < a.n_root_children; ++k) L *= fac_b[(int64_t)a.root_children[k] * a.ld + j + 1];
        const double t = log(L) + a.log_prior[j];
        s += t == ninf ? 0.0 : exp(t - m);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
    if (lane == 0) a.out[b] = m + log(s);
}

inline size_t align_up(size_t v) { return (v + 255) / 256 * 256; }

// The branch above node u under one family's lambdas
SlotParam branch_param(const cafe_ctx* c, int u, const double* lam) {
    const double l = lam[c->lam_idx[u]];
    if (!(l * 1000000000 < 9.0e18)) {                  // beyond a long: saturated on any branch (lambdas are >= 0 and not NaN here)
        SlotParam sp{};
        sp.alpha = 1.0; sp.oma2 = 0.0; sp.zero = 1;
        return sp;
    }
    return slot_param(quantize_lambda(l), quantize_time(c->blen[u]));
}
// ... and under its (lambdas, mus): either rate beyond a long saturates the branch
SlotParamLM branch_param_lm(const cafe_ctx* c, int u, const double* lam, const double* mus) {
    const double l = lam[c->lam_idx[u]], m = mus[c->lam_idx[u]];
    if (!(l * 1000000000 < 9.0e18) || !(m * 1000000000 < 9.0e18)) {
        SlotParamLM sp{};
        sp.alpha = 1.0; sp.beta = 1.0; sp.q = 0.0; sp.zero = 1;
        return sp;
    }
    return slot_param_lm(quantize_lambda(l), quantize_lambda(m), quantize_time(c->blen[u]));
}

// What the two entries differ in: the slot type (the branch kernel's argument block and launcher follow from it) and how a
// family's rates become a branch's slot.  mus is null for the lambda = mu entry.
struct EqualRates {
    using Slot = SlotParam;
    static constexpr const char* entry = "cafe_score_per_family";
    static constexpr bool reads_context_rates = true;  // lambda = mu is what it computes: refused while the context has death rates
    static Slot slot(const cafe_ctx* c, int u, const double* lam, const double*) { return branch_param(c, u, lam); }
};
struct TwoRates {
    using Slot = SlotParamLM;
    static constexpr const char* entry = "cafe_score_per_family_lm";
    static constexpr bool reads_context_rates = false;
    static Slot slot(const cafe_ctx* c, int u, const double* lam, const double* mus) { return branch_param_lm(c, u, lam, mus); }
};

// The host frame of both entries: argument checks, what the host decides alone, levels and tables, the batches under the
// workspace limit, one launch per level and the root kernel.  mus[n][n_lambdas] belongs to Kind = TwoRates only.
template <class Kind>
int per_family_frame(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, const double* mus, double* family_lnl) {
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
        if (family[i] < 0 || family[i] >= c->F_all) { set_err(c, "%s: family index %lld outside 0..%lld", who, (long long)family[i], (long long)c->F_all - 1); return CAFE_ERR_ARGUMENT; }
    if (n == 0) return CAFE_OK;
    const int nn = c->n_nodes, L = c->n_lambdas, ld = round_up(c->N, 2);

    // ---- what the host decides alone: an invalid vector is -inf (base_model.cpp:56-60); a NaN that passes is_valid stays NaN
    std::vector<int64_t> active;
    active.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double* lam = lambdas + i * L;
        bool nan = false, valid = lambdas_valid(c, lam);
        for (int k = 0; k < L; ++k) nan = nan || std::isnan(lam[k]);
        for (int k = 0; mus && k < L; ++k) valid = valid && mus[i * L + k] >= 0;      // rates_valid's rule for a death rate
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
    const size_t static_bytes = align_up(sizeof(int32_t) * tables.size()) + align_up(sizeof(double) * reals.size());
    const size_t family_bytes = sizeof(double) * (size_t)nn * ld + sizeof(Slot) * (size_t)nn + sizeof(int64_t) + sizeof(double);
    size_t budget = 0;
    HIP_TRY(c, workspace_budget(c->workspace_limit, c->pf_dev_bytes, &budget));
    int64_t batch = std::max<int64_t>(1, std::min<int64_t>(na, budget > static_bytes + 1024 ? (int64_t)((budget - static_bytes - 1024) / family_bytes) : 1));
    if (c->pf_max_batch > 0) batch = std::min(batch, c->pf_max_batch);
    const size_t o_reals = align_up(sizeof(int32_t) * tables.size()), o_col = o_reals + align_up(sizeof(double) * reals.size()),
                 o_out = o_col + align_up(sizeof(int64_t) * batch), o_slots = o_out + align_up(sizeof(double) * batch),
                 o_fac = o_slots + align_up(sizeof(Slot) * (size_t)batch * nn), need = o_fac + sizeof(double) * (size_t)batch * nn * ld;
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

    std::vector<Slot> slots((size_t)batch * nn);
    std::vector<int64_t> col((size_t)batch);
    std::vector<double> res((size_t)batch);
    for (int64_t b0 = 0; b0 < na; b0 += batch) {
        const int64_t nb = std::min(batch, na - b0);
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t i = active[b0 + b];
            col[b] = c->ref_of[family[i]];
            for (int u = 0; u < nn; ++u) slots[(size_t)b * nn + u] = u == c->root ? Slot{} : Kind::slot(c, u, lambdas + i * L, mus ? mus + i * L : nullptr);
        }
        HIP_TRY(c, hipMemcpyAsync(base + o_slots, slots.data(), sizeof(Slot) * (size_t)nb * nn, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(base + o_col, col.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
        for (int lv = 0; lv < n_levels; ++lv) {
            a.nodes = d_tables + o_level + level_off[lv];
            HIP_TRY(c, launch_family_lambda(a, c->N, nb, level_off[lv + 1] - level_off[lv], s));
        }
        if (c->root_rule == CAFE_ROOT_SUM) CAFE_LAUNCH(c, family_root_sum_kernel, dim3((unsigned)nb), dim3(64), 0, s, ra);
        else CAFE_LAUNCH(c, family_root_kernel, dim3((unsigned)nb), dim3(64), 0, s, ra);
        HIP_TRY(c, hipMemcpyAsync(res.data(), base + o_out, sizeof(double) * nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));            // the host tables of this batch go out of use
        for (int64_t b = 0; b < nb; ++b) family_lnl[active[b0 + b]] = res[b];
    }
    return CAFE_OK;
}

}  // namespace

int score_per_family_impl(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, double* family_lnl) {
    return per_family_frame<EqualRates>(c, pr, n, family, lambdas, nullptr, family_lnl);
}
int score_per_family_lm_impl(cafe_ctx* c, const cafe_params* pr, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                             double* family_lnl) {
    if (n > 0 && !mus) { set_err(c, "cafe_score_per_family_lm: mus are required"); return CAFE_ERR_ARGUMENT; }
    return per_family_frame<TwoRates>(c, pr, n, family, lambdas, mus, family_lnl);
}

}  // namespace cafe

int cafe_score_per_family(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family, const double* lambdas, double* family_lnl) {
    const int rc = cafe::guarded(ctx, "cafe_score_per_family", [&] { return cafe::score_per_family_impl(ctx, params, n, family, lambdas, family_lnl); });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

int cafe_score_per_family_lm(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family, const double* lambdas, const double* mus,
                             double* family_lnl) {
    const int rc = cafe::guarded(ctx, "cafe_score_per_family_lm", [&] { return cafe::score_per_family_lm_impl(ctx, params, n, family, lambdas, mus, family_lnl); });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}
