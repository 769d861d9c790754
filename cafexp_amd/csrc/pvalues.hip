// compute_pvalues (src/probability.cpp:255-454) entirely on the device.
//
// The reference simulates, for every root size i < R, `n` families down the tree (each child size drawn from row
// `parent size` of the branch's transition matrix restricted to sizes 0..M-1: set_weighted_random_family_size,
// :320-351), prunes every simulated family and keeps max_j L_root[j] (:273-317), sorts the n values per root size and
// reports for each observed family max_i upper_bound(conditional[i], observed) / n (:379-444).
//
// cafexp_amd/host/pvalues.cpp follows that draw for draw on the host (same engine, same libstdc++ distributions) and is
// what the parity tests compare with the reference at a fixed seed.  This file is the same computation for shapes where
// one host thread and a host copy of every matrix would dominate (100 taxa, N = 751: 148 M draws, 0.9 GB): the draws
// come from a counter-based generator (Philox4x32-10 keyed by the seed, counter = (family, node)), so the simulated
// families are a DIFFERENT sample of the same distribution: p-values agree with the reference statistically (Monte
// Carlo error ~ sqrt(p(1-p)/n)), not draw for draw.
//   row_cdf       prefix sums of every branch's row-major matrix rows over c = 0..M-1 (inverse-CDF sampling; tree_sampler.h,
//                 shared with simulate.hip like the generator and the draw)
//   simulate      one thread per simulated family, nodes parents first; sizes in a [node][family] scratch, leaves
//                 written straight into the child context's taxon-major count table
//   (prune)       cafe_score.hip's root-maximum schedule on the child context and on the observed families
//   sort_rows     bitonic sort of each root size's n values in LDS
//   tree_pvalue   per observed family: max over root sizes of the upper_bound position
#include <algorithm>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

#include "cafe_call.h"
#include "tree_sampler.h"

namespace cafe {

namespace {

struct SimArgs {
    const double* cdf;          // [slot][N][ld] row-major prefix sums
    int64_t stride;
    int32_t ld, M, n_nodes, n_sim;
    const int32_t* order;       // nodes, parents before children (root first)
    const int32_t* parent;      // [n_nodes]
    const int32_t* slot;        // [n_nodes] cdf slot of the branch above the node
    const int32_t* leaf_taxon;  // [n_nodes]
    int32_t* sizes;             // [n_nodes][ld_f] scratch
    int32_t* counts;            // child context's [taxon][counts_ld]
    int64_t counts_ld, ld_f, n_families;
    uint32_t k0, k1;
};

__global__ __launch_bounds__(256) void simulate_kernel(const SimArgs a) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= a.n_families) return;
    const int root_size = (int)(f / a.n_sim);
    for (int t = 0; t < a.n_nodes; ++t) {
        const int v = a.order[t];
        const int par = a.parent[v];
        int size;
        if (par < 0) {
            size = root_size;
        } else {
            const int ps = a.sizes[(int64_t)par * a.ld_f + f];
            size = 0;
            if (ps > 0) {                                   // an extinct lineage stays extinct, no draw (:328)
                const double* row = a.cdf + (int64_t)a.slot[v] * a.stride + (int64_t)ps * a.ld;
                size = draw_child_size(row, a.M, uniform01(f, v, 0u, a.k0, a.k1));
            }
        }
        a.sizes[(int64_t)v * a.ld_f + f] = size;
        const int tx = a.leaf_taxon[v];
        if (tx >= 0) a.counts[(int64_t)tx * a.counts_ld + f] = size;
    }
}

// one block per root size: sorts its n values ascending (n <= 2048, padded with +inf)
__global__ __launch_bounds__(256) void sort_rows_kernel(double* __restrict__ v, int n) {
    extern __shared__ double sh[];
    int P2 = 1;
    while (P2 < n) P2 <<= 1;
    double* row = v + (int64_t)blockIdx.x * n;
    for (int i = threadIdx.x; i < P2; i += 256) sh[i] = i < n ? row[i] : __builtin_inf();
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P2; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool up = (i & k) == 0;
                    const double x = sh[i], y = sh[ixj];
                    if ((x > y) == up) { sh[i] = y; sh[ixj] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < n; i += 256) row[i] = sh[i];
}

// compute_tree_pvalue: max over root sizes of pvalue(observed, conditional[s]) (probability.cpp:379-407)
__global__ __launch_bounds__(256) void tree_pvalue_kernel(const double* __restrict__ observed, int64_t F, const double* __restrict__ cond, int R, int n,
                                                          double* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const double v = observed[f];
    double best = 0.0;
    for (int s = 0; s < R; ++s) {
        const double* c = cond + (int64_t)s * n;
        int lo = 0, hi = n;                                 // first element > v
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (!(v < c[mid])) lo = mid + 1; else hi = mid;
        }
        const int idx = lo != n ? lo : n - 1;
        const double p = idx / (double)n;
        if (s == 0 || p > best) best = p;
    }
    out[f] = best;
}

// The two closing launches, one place for cafe_pvalues and the test hooks below
hipError_t launch_sort_rows(double* d_rows, int rows, int n, hipStream_t s) {
    int P2 = 1;
    while (P2 < n) P2 <<= 1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sort_rows_kernel, dim3(rows), dim3(256), sizeof(double) * P2, s, d_rows, n);
    return hipGetLastError();
}

hipError_t launch_tree_pvalue(const double* d_observed, int64_t F, const double* d_cond, int R, int n, double* d_out, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(tree_pvalue_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, d_observed, F, d_cond, R, n, d_out);
    return hipGetLastError();
}

}  // namespace

int pvalues_impl(cafe_ctx* c, const cafe_params* pr, int32_t n_sim, uint64_t seed, double* pvalues, const cafe_pvalue_stages* cap) {
    if (!pr || !pr->lambdas || !pvalues) { set_err(c, "cafe_pvalues: lambdas and pvalues are required"); return CAFE_ERR_ARGUMENT; }
    if (n_sim < 1 || n_sim > 2048) { set_err(c, "cafe_pvalues: 1..2048 simulations per root size"); return CAFE_ERR_ARGUMENT; }
    if (!rates_valid(c, pr->lambdas)) { set_err(c, "cafe_pvalues: invalid lambda or death rate"); return CAFE_ERR_ARGUMENT; }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int n = c->n_nodes, N = c->N, M = c->M, R = c->R;
    const int64_t Fs = (int64_t)R * n_sim;

    // ---- observed families: max_j L_root[j] (also builds this call's matrices for the plain lambdas)
    if (const int rc = enqueue_rootmax(c, pr->lambdas, s)) { fail_after_enqueue(c, s); return rc; }

    // ---- row-major matrix + CDF of EVERY branch (the scorer keeps interior branches k-major only)
    MatrixPool sp = row_major_pool(N);
    // (with death rates set, cafe_set_death_rates: the two-rate parameters, built by the two-rate kernel; one or the other is filled)
    const bool lm = !c->mus.empty();
    std::map<std::tuple<long, long, long>, int> key_slot;
    std::vector<SlotParam> slots;
    std::vector<SlotParamLM> slots_lm;
    std::vector<int32_t> h_slot(n, 0), h_parent(n), h_leaf(n), h_order;
    for (int v = 0; v < n; ++v) {
        h_parent[v] = c->parent[v];
        h_leaf[v] = c->leaf_taxon[v];
        if (v == c->root) continue;
        long lq, mq;
        quantized_rates(pr->lambdas, context_mus(c), c->lam_idx[v], 1.0, &lq, &mq);
        const long tq = quantize_time(c->blen[v]);
        auto it = key_slot.find({tq, lq, mq});
        if (it == key_slot.end()) {
            it = key_slot.emplace(std::make_tuple(tq, lq, mq), (int)key_slot.size()).first;
            if (lm) slots_lm.push_back(slot_param_lm(lq, mq, tq)); else slots.push_back(slot_param(lq, tq));
        }
        h_slot[v] = it->second;
    }
    for (int v = n - 1; v >= 0; --v) h_order.push_back(v);          // parents have larger indices: descending = parents first
    DevBuf d_pool, d_sp, d_meta, d_sizes, d_cond, d_pv;
    const size_t n_slots = key_slot.size();
    const size_t sp_bytes = lm ? sizeof(SlotParamLM) * n_slots : sizeof(SlotParam) * n_slots;
    const size_t pool_bytes = sizeof(double) * (size_t)sp.stride * n_slots;
    if (hipMalloc(&d_pool.p, pool_bytes) != hipSuccess || hipMalloc(&d_sp.p, sp_bytes) != hipSuccess ||
        hipMalloc(&d_meta.p, sizeof(int32_t) * 4 * n) != hipSuccess || hipMalloc(&d_cond.p, sizeof(double) * Fs) != hipSuccess ||
        hipMalloc(&d_pv.p, sizeof(double) * c->F_uniq) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "cafe_pvalues: cannot allocate the simulation workspace");
        return CAFE_ERR_MEMORY;
    }
    sp.base = static_cast<double*>(d_pool.p);
    HIP_TRY(c, hipMemsetAsync(d_pool.p, 0, pool_bytes, s));
    HIP_TRY(c, hipMemcpyAsync(d_sp.p, lm ? (const void*)slots_lm.data() : (const void*)slots.data(), sp_bytes, hipMemcpyHostToDevice, s));
    int32_t* meta = static_cast<int32_t*>(d_meta.p);
    HIP_TRY(c, hipMemcpyAsync(meta, h_order.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(meta + n, h_parent.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(meta + 2 * n, h_slot.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(meta + 3 * n, h_leaf.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    if (lm) HIP_TRY(c, launch_bd_matrix_build(sp, static_cast<const SlotParamLM*>(d_sp.p), (int)n_slots, s));
    else HIP_TRY(c, launch_bd_matrix_build(sp, static_cast<const SlotParam*>(d_sp.p), (int)n_slots, s));
    HIP_TRY(c, launch_row_cdf(sp.base, sp.stride, sp.ld, (int)n_slots, N, M, s));
    HIP_TRY(c, hipStreamSynchronize(s));                            // the host vectors above go out of use

    // ---- simulate into a child context over the same tree, prune, keep the root maxima
    cafe_ctx* child = create_child_for_device_counts(c, Fs);
    if (!child) { set_err(c, "cafe_pvalues: cannot create the context of %lld simulated families", (long long)Fs); return CAFE_ERR_MEMORY; }
    struct ChildGuard { cafe_ctx* p; ~ChildGuard() { destroy_child(p); } } guard{child};
    if (lm) { const int rc = set_death_rates_impl(child, c->mus.data()); if (rc != CAFE_OK) { set_err(c, "cafe_pvalues: %s", child->err.c_str()); return rc; } }
    if (hipMalloc(&d_sizes.p, sizeof(int32_t) * (size_t)n * Fs) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "cafe_pvalues: cannot allocate the simulation scratch");
        return CAFE_ERR_MEMORY;
    }
    SimArgs a{};
    a.cdf = sp.base; a.stride = sp.stride; a.ld = sp.ld; a.M = M; a.n_nodes = n; a.n_sim = n_sim;
    a.order = meta; a.parent = meta + n; a.slot = meta + 2 * n; a.leaf_taxon = meta + 3 * n;
    a.sizes = static_cast<int32_t*>(d_sizes.p); a.counts = child->d_counts; a.counts_ld = child->Fp; a.ld_f = Fs; a.n_families = Fs;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    CAFE_LAUNCH(c, simulate_kernel, dim3((unsigned)((Fs + 255) / 256)), dim3(256), 0, s, a);
    HIP_TRY(c, hipStreamSynchronize(s));                            // the child context runs on its own stream
    if (cap && cap->sizes) HIP_TRY(c, hipMemcpy(cap->sizes, d_sizes.p, sizeof(int32_t) * (size_t)n * Fs, hipMemcpyDeviceToHost));
    if (cap && cap->counts)
        HIP_TRY(c, hipMemcpy2D(cap->counts, sizeof(int32_t) * Fs, child->d_counts, sizeof(int32_t) * child->Fp, sizeof(int32_t) * Fs, c->n_taxa, hipMemcpyDeviceToHost));
    if (const int rc = enqueue_rootmax(child, pr->lambdas, child->stream)) {
        fail_after_enqueue(child, child->stream);
        fail_after_enqueue(c, s);                                   // (the observed families' root maxima are not results of a failed call)
        set_err(c, "cafe_pvalues: %s", child->err.c_str());
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(d_cond.p, child->d_fam_out, sizeof(double) * Fs, hipMemcpyDeviceToDevice, child->stream));
    if (cap && cap->cond_unsorted) {
        HIP_TRY(c, hipStreamSynchronize(child->stream));
        HIP_TRY(c, hipMemcpy(cap->cond_unsorted, d_cond.p, sizeof(double) * Fs, hipMemcpyDeviceToHost));
    }
    HIP_TRY(c, launch_sort_rows(static_cast<double*>(d_cond.p), R, n_sim, child->stream));
    HIP_TRY(c, hipStreamSynchronize(child->stream));
    child->upload_pending = false;
    if (cap && cap->cond_sorted) HIP_TRY(c, hipMemcpy(cap->cond_sorted, d_cond.p, sizeof(double) * Fs, hipMemcpyDeviceToHost));

    // ---- p-value of every (distinct) observed family, spread to the families that share a column
    HIP_TRY(c, launch_tree_pvalue(c->d_fam_out, c->F_uniq, static_cast<const double*>(d_cond.p), R, n_sim, static_cast<double*>(d_pv.p), s));
    std::vector<double> tmp((size_t)c->F_uniq);
    HIP_TRY(c, hipMemcpyAsync(tmp.data(), d_pv.p, sizeof(double) * c->F_uniq, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->upload_pending = false;
    spread_unique(c, tmp.data(), pvalues);
    if (cap && cap->observed) {
        HIP_TRY(c, hipMemcpy(tmp.data(), c->d_fam_out, sizeof(double) * c->F_uniq, hipMemcpyDeviceToHost));
        spread_unique(c, tmp.data(), cap->observed);
    }
    return CAFE_OK;
}

// A test hook's frame: host arrays to the device, one launch on the null stream, the result back
namespace {

int on_device(int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return CAFE_ERR_DEVICE;
    return hipSetDevice(device) == hipSuccess ? CAFE_OK : CAFE_ERR_DEVICE;
}

}  // namespace

int debug_sort_rows(int32_t device, double* values, int32_t rows, int32_t n) {
    if (!values || rows < 1 || n < 1 || n > 2048) return CAFE_ERR_ARGUMENT;
    if (const int rc = on_device(device)) return rc;
    const size_t bytes = sizeof(double) * (size_t)rows * n;
    DevBuf d;
    if (hipMalloc(&d.p, bytes) != hipSuccess) { (void)hipGetLastError(); return CAFE_ERR_MEMORY; }
    if (hipMemcpy(d.p, values, bytes, hipMemcpyHostToDevice) != hipSuccess) return CAFE_ERR_DEVICE;
    if (launch_sort_rows(static_cast<double*>(d.p), rows, n, nullptr) != hipSuccess) return CAFE_ERR_DEVICE;
    return hipMemcpy(values, d.p, bytes, hipMemcpyDeviceToHost) == hipSuccess ? CAFE_OK : CAFE_ERR_DEVICE;
}

int debug_tree_pvalue(int32_t device, const double* observed, int64_t F, const double* cond, int32_t R, int32_t n, double* pvalues) {
    if (!observed || !cond || !pvalues || F < 1 || R < 1 || n < 1 || n > 2048) return CAFE_ERR_ARGUMENT;
    if (const int rc = on_device(device)) return rc;
    DevBuf d_obs, d_cond, d_pv;
    if (hipMalloc(&d_obs.p, sizeof(double) * F) != hipSuccess || hipMalloc(&d_cond.p, sizeof(double) * (size_t)R * n) != hipSuccess ||
        hipMalloc(&d_pv.p, sizeof(double) * F) != hipSuccess) {
        (void)hipGetLastError();
        return CAFE_ERR_MEMORY;
    }
    if (hipMemcpy(d_obs.p, observed, sizeof(double) * F, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_cond.p, cond, sizeof(double) * (size_t)R * n, hipMemcpyHostToDevice) != hipSuccess)
        return CAFE_ERR_DEVICE;
    if (launch_tree_pvalue(static_cast<const double*>(d_obs.p), F, static_cast<const double*>(d_cond.p), R, n, static_cast<double*>(d_pv.p), nullptr) != hipSuccess)
        return CAFE_ERR_DEVICE;
    return hipMemcpy(pvalues, d_pv.p, sizeof(double) * F, hipMemcpyDeviceToHost) == hipSuccess ? CAFE_OK : CAFE_ERR_DEVICE;
}

}  // namespace cafe

extern "C" int cafe_pvalues(cafe_ctx* ctx, const cafe_params* params, int32_t n_simulations, uint64_t seed, double* pvalues) {
    return cafe::guarded_observed(ctx, "cafe_pvalues", [&] { return cafe::pvalues_impl(ctx, params, n_simulations, seed, pvalues); });
}

extern "C" int cafe_debug_pvalues_stages(cafe_ctx* ctx, const cafe_params* params, int32_t n_simulations, uint64_t seed,
                                         const cafe_pvalue_stages* stages, double* pvalues) {
    return cafe::guarded_observed(ctx, "cafe_debug_pvalues_stages", [&] { return cafe::pvalues_impl(ctx, params, n_simulations, seed, pvalues, stages); });
}

extern "C" int cafe_debug_sort_rows(int32_t device, double* values, int32_t rows, int32_t n) {
    try { return cafe::debug_sort_rows(device, values, rows, n); } catch (const std::exception&) { return CAFE_ERR_MEMORY; }
}

extern "C" int cafe_debug_tree_pvalue(int32_t device, const double* observed, int64_t n_observed, const double* cond, int32_t n_root_sizes,
                                      int32_t n, double* pvalues) {
    try { return cafe::debug_tree_pvalue(device, observed, n_observed, cond, n_root_sizes, n, pvalues); } catch (const std::exception&) { return CAFE_ERR_MEMORY; }
}
