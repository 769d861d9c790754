// cafe_simulate: the reference's simulator (-s; src/simulator.cpp:62-103, src/probability.cpp:320-377) on the device.
//
// The reference draws every family on one host thread from std::discrete_distribution objects it rebuilds per draw, and
// rebuilds a matrix_cache every LAMBDA_PERTURBATION_STEP_SIZE families -- for the base model too, whose lambda never
// changes.  Here:
//   batches     the chunks (chunk_size families sharing one lambda multiplier) are cut into batches whose matrices and
//               buffers fit the workspace; within a batch, chunks whose quantized lambdas agree share one block of
//               matrices (the base model: one block for the whole batch)
//   K1          launch_bd_matrix_build, row-major, order S, one slot per (block, distinct (lambda index, t_q) pair);
//               cafe_simulate_lm with death rates: the same launcher on slot_param_lm slots, the multiplier scaling both rates, and
//               chunks share a block when both quantized vectors agree.  Everything behind the matrices is the same code
//   row_cdf     inclusive prefix sums of rows 1..S-1 over columns 0..S-1 (the reference's weights, :338-341); this pass, the
//               generator and the draw are tree_sampler.h's, shared with pvalues.hip
//   sample      one thread per family, nodes parents first, inverse-CDF draws by binary search; sizes node-major in a
//               scratch table so that a parent's size is one coalesced load
//   transpose   the scratch to family-major leaf counts / node sizes through LDS, so that both writes coalesce
// Every draw is Philox4x32-10(counter = (family lo, family hi, node, stream), key = seed): stream 0 is the child-size
// draw, stream 1 the error-model draw.  A result therefore depends on the arguments only, never on the batch cut.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "cafe_ctx.h"
#include "tree_sampler.h"

namespace cafe {

namespace {

constexpr int kTile = 64;                       // families x columns per transpose tile

struct SampleArgs {
    const double* cdf;              // [slot][S][ld] row prefix sums
    int64_t stride;
    int32_t ld, S, n_nodes, n_pairs;
    const int32_t* order;           // nodes, parents first
    const int32_t* parent;          // [n_nodes]
    const int32_t* pair_of;         // [n_nodes] matrix pair of the branch above the node
    const int32_t* is_leaf;         // [n_nodes]
    const int32_t* chunk_block;     // [chunks of the batch] matrix block of the chunk
    const int32_t* root_size;       // [n_families] (whole problem)
    const double* err;              // [S][n_dev] or nullptr
    int32_t n_dev, err_max;
    int32_t* flag;                  // set to 1 when a leaf size is outside the error model
    int32_t* sizes;                 // [n_nodes][fb] scratch
    int64_t f0, fb, chunk_size, chunk0;
    uint32_t k0, k1;
};

__global__ __launch_bounds__(256) void sample_kernel(const SampleArgs a) {
    const int64_t fl = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (fl >= a.fb) return;
    const int64_t f = a.f0 + fl;
    const int64_t slot_base = (int64_t)a.chunk_block[f / a.chunk_size - a.chunk0] * a.n_pairs;
    for (int t = 0; t < a.n_nodes; ++t) {
        const int v = a.order[t];
        const int par = a.parent[v];
        int size;
        if (par < 0) {
            size = a.root_size[f];
        } else {
            const int ps = a.sizes[(int64_t)par * a.fb + fl];
            size = 0;
            if (ps > 0) {                               // an extinct lineage stays extinct, no draw (:328)
                const double* row = a.cdf + (slot_base + a.pair_of[v]) * a.stride + (int64_t)ps * a.ld;
                size = draw_child_size(row, a.S, uniform01(f, v, 0u, a.k0, a.k1));
            }
            if (a.err && a.is_leaf[v]) {                // adjust_for_error_model (:354-377)
                if (size >= a.err_max) {
                    *a.flag = 1;
                } else {
                    const double* probs = a.err + (int64_t)size * a.n_dev;
                    const double u = uniform01(f, v, 1u, a.k0, a.k1);
                    if (u < probs[0]) --size;
                    else if (u > 1 - probs[2]) ++size;
                }
            }
        }
        a.sizes[(int64_t)v * a.fb + fl] = size;
    }
}

// out[(f0 + fl) * W + j] = sizes[src[j]][fl]: 64 families x 64 columns per block through LDS
__global__ __launch_bounds__(256) void transpose_kernel(const int32_t* __restrict__ sizes, int64_t fb, const int32_t* __restrict__ src, int W,
                                                        int32_t* __restrict__ out) {
    __shared__ int32_t tile[kTile][kTile + 1];          // [column][family]
    const int64_t fbase = (int64_t)blockIdx.x * kTile;
    const int j0 = blockIdx.y * kTile;
    const int nf = (int)min<int64_t>(kTile, fb - fbase), nj = min(kTile, W - j0);
    for (int i = threadIdx.x; i < kTile * kTile; i += 256) {
        const int j = i / kTile, fl = i % kTile;         // read along families: coalesced
        if (j < nj && fl < nf) tile[j][fl] = sizes[(int64_t)src[j0 + j] * fb + fbase + fl];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nf * nj; i += 256) {
        const int fl = i / nj, j = i % nj;               // write along the row segment
        out[(fbase + fl) * W + j0 + j] = tile[j][fl];
    }
}

struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};

void put_err(char* err, size_t errlen, const char* fmt, ...) {
    if (!err || !errlen) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, errlen, fmt, ap);
    va_end(ap);
}

#define SIM_TRY(expr)                                                                                            \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                  \
            put_err(err, errlen, "%s: %s failed: %s (%s:%d)", who, #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return CAFE_ERR_DEVICE;                                                                              \
        }                                                                                                        \
    } while (0)

// The quantized lambda of every lambda index under multiplier m (matrix_cache_key, matrix_cache.h:47): chunks with equal
// vectors build the same matrices.
// With death rates the key is [lambdas..., mus...].
std::vector<long> chunk_key(const cafe_sim_problem* p, const double* mus, double m) {
    const int L = p->n_lambdas;
    std::vector<long> k((size_t)L * (mus ? 2 : 1));
    for (int i = 0; i < L; ++i) k[i] = quantize_lambda(p->lambdas[i] * m);
    for (int i = 0; mus && i < L; ++i) k[L + i] = quantize_lambda(mus[i] * m);
    return k;
}

// mus == nullptr: cafe_simulate (lambda = mu, K1)
int simulate_impl(const cafe_sim_problem* p, const double* mus, uint64_t seed, int32_t* leaf_counts, int32_t* node_sizes, char* err, size_t errlen) {
    const char* const who = mus ? "cafe_simulate_lm" : "cafe_simulate";      // the entry the messages name
    // ---------------------------------------------------------------- arguments
    if (!p) { put_err(err, errlen, "%s: problem is NULL", who); return CAFE_ERR_ARGUMENT; }
    const int n = p->n_nodes, S = p->max_family_size, T = p->n_taxa, L = p->n_lambdas;
    const int64_t F = p->n_families;
    if (n < 2 || !p->parent || !p->branch_length || !p->leaf_taxon || T < 1) { put_err(err, errlen, "%s: a tree of >= 2 nodes with parent, branch_length and leaf_taxon is required", who); return CAFE_ERR_ARGUMENT; }
    if (S < 2 || S > bd_matrix_max_order()) { put_err(err, errlen, "%s: matrix order %d outside 2..%d", who, S, bd_matrix_max_order()); return CAFE_ERR_ARGUMENT; }
    if (F < 0 || (F > 0 && !p->root_size)) { put_err(err, errlen, "%s: root_size[n_families] is required", who); return CAFE_ERR_ARGUMENT; }
    if (!leaf_counts && !node_sizes) { put_err(err, errlen, "%s: no output", who); return CAFE_ERR_ARGUMENT; }
    if (L < 1 || !p->lambdas) { put_err(err, errlen, "%s: lambdas are required", who); return CAFE_ERR_ARGUMENT; }
    for (int i = 0; i < L; ++i) {
        const double l = p->lambdas[i];
        if (!std::isfinite(l) || l < 0 || (L == 1 && !(l > 0)) || l * 1000000000 > 1e18) { put_err(err, errlen, "%s: invalid lambda %g", who, l); return CAFE_ERR_ARGUMENT; }
    }
    for (int i = 0; mus && i < L; ++i) {
        const double mu = mus[i];
        if (!std::isfinite(mu) || mu < 0 || mu * 1000000000 > 1e18) { put_err(err, errlen, "%s: invalid mu %g", who, mu); return CAFE_ERR_ARGUMENT; }
    }
    if (p->chunk_size < 0) { put_err(err, errlen, "%s: chunk_size < 0", who); return CAFE_ERR_ARGUMENT; }
    const int64_t chunk = p->chunk_size > 0 ? p->chunk_size : std::max<int64_t>(F, 1);
    const int64_t n_chunks = (F + chunk - 1) / chunk;
    double max_lambda = 0;
    for (int i = 0; i < L; ++i) max_lambda = std::max(max_lambda, p->lambdas[i]);
    double max_mu = 0;
    for (int i = 0; mus && i < L; ++i) max_mu = std::max(max_mu, mus[i]);
    if (p->chunk_multiplier)
        for (int64_t c = 0; c < n_chunks; ++c) {
            const double m = p->chunk_multiplier[c];
            if (!std::isfinite(m) || m < 0 || max_lambda * m * 1000000000 > 1e18) { put_err(err, errlen, "%s: invalid lambda multiplier %g of chunk %lld", who, m, (long long)c); return CAFE_ERR_ARGUMENT; }
            if (max_mu * m * 1000000000 > 1e18) { put_err(err, errlen, "%s: mu %g times multiplier %g of chunk %lld is out of range", who, max_mu, m, (long long)c); return CAFE_ERR_ARGUMENT; }
        }
    if (p->error_model && (p->n_deviations < 3 || p->error_model_max_size < 0)) { put_err(err, errlen, "%s: an error model needs >= 3 deviations", who); return CAFE_ERR_ARGUMENT; }
    int root = -1;
    std::vector<int32_t> n_children(n, 0);
    for (int v = 0; v < n; ++v) {
        const int par = p->parent[v];
        if (par < 0) { if (root >= 0) { put_err(err, errlen, "%s: more than one root", who); return CAFE_ERR_ARGUMENT; } root = v; continue; }
        if (par <= v || par >= n) { put_err(err, errlen, "%s: node %d: parents must come after their children", who, v); return CAFE_ERR_ARGUMENT; }
        ++n_children[par];
        const double t = p->branch_length[v];
        if (!std::isfinite(t) || t < 0 || t > 1e15) { put_err(err, errlen, "%s: invalid branch length %g", who, t); return CAFE_ERR_ARGUMENT; }
        if (p->lambda_index && (p->lambda_index[v] < 0 || p->lambda_index[v] >= L)) { put_err(err, errlen, "%s: lambda index out of range", who); return CAFE_ERR_ARGUMENT; }
    }
    if (root < 0) { put_err(err, errlen, "%s: no root", who); return CAFE_ERR_ARGUMENT; }
    std::vector<int32_t> taxon_node(T, -1), is_leaf(n, 0);
    for (int v = 0; v < n; ++v) {
        const int tx = p->leaf_taxon[v];
        if ((n_children[v] == 0) != (tx >= 0) || tx >= T || (tx >= 0 && taxon_node[tx] >= 0)) {
            put_err(err, errlen, "%s: leaf_taxon must name a distinct taxon for every leaf and -1 for interior nodes", who);
            return CAFE_ERR_ARGUMENT;
        }
        if (tx >= 0) { taxon_node[tx] = v; is_leaf[v] = 1; }
    }
    for (int t = 0; t < T; ++t) if (taxon_node[t] < 0) { put_err(err, errlen, "%s: taxon %d has no leaf", who, t); return CAFE_ERR_ARGUMENT; }
    for (int64_t f = 0; f < F; ++f)
        if (p->root_size[f] < 0 || p->root_size[f] >= S) {
            put_err(err, errlen, "%s: root size %d of family %lld outside 0..%d", who, p->root_size[f], (long long)f, S - 1);
            return CAFE_ERR_ARGUMENT;
        }
    if (F == 0) return CAFE_OK;

    // ---------------------------------------------------------------- static tables
    // matrix pairs: distinct (lambda index, t_q) of the branches (matrix_cache_key without the multiplier)
    std::map<std::pair<int, long>, int> pair_id;
    std::vector<int32_t> pair_of(n, 0), pair_lam, order;
    std::vector<long> pair_tq;
    for (int v = 0; v < n; ++v) {
        if (v == root) continue;
        const int li = p->lambda_index ? p->lambda_index[v] : 0;
        const long tq = quantize_time(p->branch_length[v]);
        auto it = pair_id.find({li, tq});
        if (it == pair_id.end()) {
            it = pair_id.emplace(std::make_pair(li, tq), (int)pair_lam.size()).first;
            pair_lam.push_back(li);
            pair_tq.push_back(tq);
        }
        pair_of[v] = it->second;
    }
    for (int v = n - 1; v >= 0; --v) order.push_back(v);              // parents have larger indices: parents first
    const int n_pairs = (int)pair_lam.size();
    std::vector<int32_t> all_nodes(n);
    for (int v = 0; v < n; ++v) all_nodes[v] = v;

    MatrixPool pool = row_major_pool(S);
    const size_t slot_bytes = mus ? sizeof(SlotParamLM) : sizeof(SlotParam);
    const size_t block_bytes = sizeof(double) * (size_t)pool.stride * n_pairs + slot_bytes * n_pairs + sizeof(int32_t);
    const size_t family_bytes = sizeof(int32_t) * ((size_t)n + (leaf_counts ? T : 0) + (node_sizes ? n : 0));

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || p->device < 0 || p->device >= ndev) { put_err(err, errlen, "%s: no HIP device %d", who, p->device); return CAFE_ERR_DEVICE; }
    SIM_TRY(hipSetDevice(p->device));
    size_t budget = 0;
    SIM_TRY(workspace_budget(p->workspace_limit, 0, &budget));
    // a batch holds <= max_blocks matrix blocks and <= max_fams families (at least one block and one tile of families)
    const int64_t max_blocks = std::max<int64_t>(1, (int64_t)(budget / 2 / block_bytes));
    const int64_t max_fams = std::max<int64_t>(kTile, (int64_t)(budget / 2 / family_bytes) / kTile * kTile);

    // ---------------------------------------------------------------- device buffers sized for the largest batch
    DevBuf d_pool, d_slots, d_meta, d_root, d_err, d_flag, d_sizes, d_leaf, d_node, d_cblock;
    StreamGuard sg;
    SIM_TRY(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    hipStream_t s = sg.s;
    const int64_t fb_max = std::min<int64_t>(F, max_fams);
    const int64_t blocks_max = std::min<int64_t>(max_blocks, n_chunks);
    const int64_t chunks_max = std::min<int64_t>(n_chunks, fb_max / chunk + 2);
    const size_t em_len = p->error_model ? (size_t)S * p->n_deviations : 0;
    const size_t meta_len = (size_t)5 * n + T;
    const bool ok =
        hipMalloc(&d_pool.p, sizeof(double) * (size_t)pool.stride * n_pairs * blocks_max) == hipSuccess &&
        hipMalloc(&d_slots.p, slot_bytes * (size_t)n_pairs * blocks_max) == hipSuccess &&
        hipMalloc(&d_meta.p, sizeof(int32_t) * meta_len) == hipSuccess &&
        hipMalloc(&d_root.p, sizeof(int32_t) * (size_t)F) == hipSuccess &&
        (!em_len || hipMalloc(&d_err.p, sizeof(double) * em_len) == hipSuccess) &&
        hipMalloc(&d_flag.p, sizeof(int32_t)) == hipSuccess &&
        hipMalloc(&d_sizes.p, sizeof(int32_t) * (size_t)n * fb_max) == hipSuccess &&
        (!leaf_counts || hipMalloc(&d_leaf.p, sizeof(int32_t) * (size_t)T * fb_max) == hipSuccess) &&
        (!node_sizes || hipMalloc(&d_node.p, sizeof(int32_t) * (size_t)n * fb_max) == hipSuccess) &&
        hipMalloc(&d_cblock.p, sizeof(int32_t) * (size_t)chunks_max) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        put_err(err, errlen, "%s: cannot allocate the workspace (%lld families, %lld matrix blocks per batch)", who, (long long)fb_max, (long long)blocks_max);
        return CAFE_ERR_MEMORY;
    }
    int32_t* meta = static_cast<int32_t*>(d_meta.p);                   // order, parent, pair_of, is_leaf, nodes, taxon_node
    std::vector<int32_t> h_meta;
    h_meta.reserve(meta_len);
    h_meta.insert(h_meta.end(), order.begin(), order.end());
    h_meta.insert(h_meta.end(), p->parent, p->parent + n);
    h_meta.insert(h_meta.end(), pair_of.begin(), pair_of.end());
    h_meta.insert(h_meta.end(), is_leaf.begin(), is_leaf.end());
    h_meta.insert(h_meta.end(), all_nodes.begin(), all_nodes.end());
    h_meta.insert(h_meta.end(), taxon_node.begin(), taxon_node.end());
    SIM_TRY(hipMemcpyAsync(meta, h_meta.data(), sizeof(int32_t) * meta_len, hipMemcpyHostToDevice, s));
    SIM_TRY(hipMemcpyAsync(d_root.p, p->root_size, sizeof(int32_t) * (size_t)F, hipMemcpyHostToDevice, s));
    if (em_len) SIM_TRY(hipMemcpyAsync(d_err.p, p->error_model, sizeof(double) * em_len, hipMemcpyHostToDevice, s));
    SIM_TRY(hipMemsetAsync(d_flag.p, 0, sizeof(int32_t), s));

    SampleArgs a{};
    a.stride = pool.stride; a.ld = pool.ld; a.S = S; a.n_nodes = n; a.n_pairs = n_pairs;
    a.order = meta; a.parent = meta + n; a.pair_of = meta + 2 * n; a.is_leaf = meta + 3 * n;
    a.chunk_block = static_cast<const int32_t*>(d_cblock.p);
    a.root_size = static_cast<const int32_t*>(d_root.p);
    a.err = em_len ? static_cast<const double*>(d_err.p) : nullptr;
    a.n_dev = p->n_deviations; a.err_max = p->error_model_max_size;
    a.flag = static_cast<int32_t*>(d_flag.p);
    a.sizes = static_cast<int32_t*>(d_sizes.p);
    a.chunk_size = chunk;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);

    // ---------------------------------------------------------------- batches
    std::vector<SlotParam> slots;
    std::vector<SlotParamLM> slots_lm;
    std::vector<int32_t> cblock;
    for (int64_t f0 = 0; f0 < F;) {
        int64_t f1 = std::min(F, f0 + fb_max);
        const int64_t c0 = f0 / chunk;
        std::map<std::vector<long>, int> block_of;
        std::vector<std::vector<long>> blocks;
        cblock.clear();
        double prev_m = std::nan("");
        for (int64_t c = c0; c * chunk < f1; ++c) {
            const double m = p->chunk_multiplier ? p->chunk_multiplier[c] : 1.0;
            if (!cblock.empty() && m == prev_m) { cblock.push_back(cblock.back()); continue; }
            prev_m = m;
            std::vector<long> key = chunk_key(p, mus, m);
            auto it = block_of.find(key);
            if (it == block_of.end()) {
                if ((int64_t)blocks.size() == blocks_max) { f1 = c * chunk; break; }     // the batch ends before this chunk
                it = block_of.emplace(key, (int)blocks.size()).first;
                blocks.push_back(key);
            }
            cblock.push_back(it->second);
        }
        const int64_t fb = f1 - f0;
        const int n_slots = (int)blocks.size() * n_pairs;
        pool.base = static_cast<double*>(d_pool.p);
        // K1 (either instantiation) stores every row of every slot (a saturated one too): no clearing pass; columns >= S are never read
        if (mus) {
            slots_lm.assign((size_t)n_slots, SlotParamLM{});
            for (size_t b = 0; b < blocks.size(); ++b)
                for (int q = 0; q < n_pairs; ++q) slots_lm[b * n_pairs + q] = slot_param_lm(blocks[b][pair_lam[q]], blocks[b][L + pair_lam[q]], pair_tq[q]);
            SIM_TRY(hipMemcpyAsync(d_slots.p, slots_lm.data(), sizeof(SlotParamLM) * n_slots, hipMemcpyHostToDevice, s));
            SIM_TRY(launch_bd_matrix_build(pool, static_cast<const SlotParamLM*>(d_slots.p), n_slots, s));
        } else {
            slots.assign((size_t)n_slots, SlotParam{});
            for (size_t b = 0; b < blocks.size(); ++b)
                for (int q = 0; q < n_pairs; ++q) slots[b * n_pairs + q] = slot_param(blocks[b][pair_lam[q]], pair_tq[q]);
            SIM_TRY(hipMemcpyAsync(d_slots.p, slots.data(), sizeof(SlotParam) * n_slots, hipMemcpyHostToDevice, s));
            SIM_TRY(launch_bd_matrix_build(pool, static_cast<const SlotParam*>(d_slots.p), n_slots, s));
        }
        SIM_TRY(hipMemcpyAsync(d_cblock.p, cblock.data(), sizeof(int32_t) * cblock.size(), hipMemcpyHostToDevice, s));
        SIM_TRY(launch_row_cdf(pool.base, pool.stride, pool.ld, n_slots, S, S, s));
        a.cdf = pool.base; a.f0 = f0; a.fb = fb; a.chunk0 = c0;
        hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((fb + 255) / 256)), dim3(256), 0, s, a);
        SIM_TRY(hipGetLastError());
        const unsigned tiles = (unsigned)((fb + kTile - 1) / kTile);
        if (leaf_counts) {
            hipLaunchKernelGGL(transpose_kernel, dim3(tiles, (T + kTile - 1) / kTile), dim3(256), 0, s, a.sizes, fb, meta + 5 * n, T,
                               static_cast<int32_t*>(d_leaf.p));
            SIM_TRY(hipGetLastError());
            SIM_TRY(hipMemcpyAsync(leaf_counts + f0 * T, d_leaf.p, sizeof(int32_t) * (size_t)fb * T, hipMemcpyDeviceToHost, s));
        }
        if (node_sizes) {
            hipLaunchKernelGGL(transpose_kernel, dim3(tiles, (n + kTile - 1) / kTile), dim3(256), 0, s, a.sizes, fb, meta + 4 * n, n,
                               static_cast<int32_t*>(d_node.p));
            SIM_TRY(hipGetLastError());
            SIM_TRY(hipMemcpyAsync(node_sizes + f0 * n, d_node.p, sizeof(int32_t) * (size_t)fb * n, hipMemcpyDeviceToHost, s));
        }
        SIM_TRY(hipStreamSynchronize(s));                              // host tables of this batch go out of use
        f0 = f1;
    }
    int32_t flag = 0;
    SIM_TRY(hipMemcpyAsync(&flag, d_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SIM_TRY(hipStreamSynchronize(s));
    if (flag) {                                                        // probability.cpp:361
        put_err(err, errlen, "Trying to simulate leaf family size that was not included in error model");
        return CAFE_ERR_ARGUMENT;
    }
    return CAFE_OK;
}

}  // namespace

}  // namespace cafe

int cafe_simulate_lm(const cafe_sim_problem* problem, const double* mus, uint64_t seed, int32_t* leaf_counts, int32_t* node_sizes, char* err,
                     size_t errlen) {
    if (err && errlen) err[0] = 0;
    try {
        return cafe::simulate_impl(problem, mus, seed, leaf_counts, node_sizes, err, errlen);
    } catch (const std::exception& e) {
        cafe::put_err(err, errlen, "%s: %s", mus ? "cafe_simulate_lm" : "cafe_simulate", e.what());
        return CAFE_ERR_MEMORY;
    }
}

int cafe_simulate(const cafe_sim_problem* problem, uint64_t seed, int32_t* leaf_counts, int32_t* node_sizes, char* err, size_t errlen) {
    return cafe_simulate_lm(problem, nullptr, seed, leaf_counts, node_sizes, err, errlen);
}
