// Ancestral histories drawn from the posterior (cafe_sample_histories): whole assignments of a size to
// every node of a family's tree, drawn top-down from the conditionals that the up pass of the marginal reconstruction
// (sum_product.h; B, F and P as in marginal.hip's header comment) makes available:
//   category  k   ~ cat_probs[k] Z_k,              Z_k = sum_{s=1..R} prior[s-1] B_root^k[s]
//   root      s   ~ prior[s-1] B_root^k[s],        s = 1..R
//   interior  j   ~ P_v^k[i][j] B_v^k[j],          j = 0..M, i the size its parent drew (row 0 of P is e_0: j = 0)
//   leaf      c   ~ err[x][t] P_v^k[i][c]          over the taps of its observed count x (no error model: c = x, no draw)
// Every draw is inverse-CDF: the first index whose inclusive prefix sum reaches u * total (tree_sampler.h, draw_child_size),
// u = uniform01(family, node, 2 * draw [+ 1 for the category], seed).  The counter carries the family's index in the table,
// so the families that share a panel column still draw their own histories, and nothing depends on batches or launch shape.
//
// One thread owns one (family, draw) -- a unit -- and walks the sizes from 0 with a running prefix until its crossing.  The
// draws of a family are neighbouring lanes: they read the same column of B_v (one address per wave and step) and, because
// the posterior clusters the parent sizes, neighbouring entries of row j of the k-major matrix (Pt[j][i-1] = P[i][j]).
// The walk stops at the crossing, which lies near the node's posterior mode -- far below M for most families.  The loads of
// eight steps are issued together, the prefix is summed in index order.  The total of an interior draw is the F_v[i] that
// the up pass stored.
#include <cmath>
#include <string>
#include <vector>

#include "sum_product.h"
#include "tree_sampler.h"

namespace cafe {

namespace {

constexpr int kWalk = 8;                 // steps whose loads are in flight together

// The units of a pass: unit = fi * n_draws + dl is draw d0 + dl of the fi-th family of the column batch
struct Units {
    const int64_t* family;               // [families of the batch] index in the problem's table
    const int32_t* column;               // [families of the batch] column of the batch's panels
    int64_t n_units;
    int n_draws, d0;                     // draws of this pass, first draw
    uint32_t k0, k1;                     // seed lo, hi
    int32_t* cat;                        // [unit] category, -1: a failed family
    int32_t* sizes;                      // [node][unit]
};

// Zk[k][f] = sum_s prior[s-1] B_root[s][f], summed in the order the root draw walks
__global__ __launch_bounds__(256) void history_rootz_kernel(const double* __restrict__ B, const double* __restrict__ prior, int R, int64_t ld,
                                                            double* __restrict__ Zk) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double z = 0.0;
    for (int s = 1; s <= R; ++s) z += prior[s - 1] * B[(int64_t)s * ld + f];
    Zk[f] = z;
}

// Z[f] = sum_k p_k Zk[k][f]
__global__ __launch_bounds__(256) void history_z_kernel(const double* __restrict__ Zk, const double* __restrict__ probs, int K, int64_t cols, int64_t ld,
                                                        double* __restrict__ Z) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double z = 0.0;
    for (int k = 0; k < K; ++k) z += probs[k] * Zk[(int64_t)k * cols + f];
    Z[f] = z;
}

// The category of every unit: the first k whose prefix of p_k Z_k reaches u * Z; -1 for a failed family
__global__ __launch_bounds__(256) void history_category_kernel(const Units un, const double* __restrict__ Zk, const double* __restrict__ probs, int K,
                                                               int64_t cols, int root) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= un.n_units) return;
    const int64_t fi = unit / un.n_draws;
    const int d = un.d0 + (int)(unit - fi * un.n_draws);
    const int col = un.column[fi];
    double z = 0.0;
    for (int k = 0; k < K; ++k) z += probs[k] * Zk[(int64_t)k * cols + col];
    int cat = -1;
    if (!evidence_failed(z)) {
        cat = 0;
        if (K > 1) {
            const double target = uniform01(un.family[fi], root, 2u * (uint32_t)d + 1u, un.k0, un.k1) * z;
            double pre = 0.0;
            cat = K - 1;
            for (int k = 0; k < K; ++k) {
                pre += probs[k] * Zk[(int64_t)k * cols + col];
                if (pre >= target) { cat = k; break; }
            }
        }
    }
    un.cat[unit] = cat;
}

// The root's size of the units of category k: s = 1..R over prior[s-1] B_root[s]; a failed family's units get -1
__global__ __launch_bounds__(256) void history_root_kernel(const Units un, int k, const double* __restrict__ B, const double* __restrict__ prior, int R,
                                                           int64_t ld, const double* __restrict__ Zk, int root) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= un.n_units) return;
    const int cat = un.cat[unit];
    int32_t* out = un.sizes + (int64_t)root * un.n_units + unit;
    if (cat < 0) { *out = -1; return; }
    if (cat != k) return;
    const int64_t fi = unit / un.n_draws;
    const int d = un.d0 + (int)(unit - fi * un.n_draws);
    const int col = un.column[fi];
    const double target = uniform01(un.family[fi], root, 2u * (uint32_t)d, un.k0, un.k1) * Zk[col];
    const double* b = B + col;
    double pre = 0.0;
    int got = R;
    for (int s0 = 1; s0 <= R; s0 += kWalk) {
        double w[kWalk];
#pragma unroll
        for (int q = 0; q < kWalk; ++q) {
            const int s = s0 + q;
            w[q] = s <= R ? prior[s - 1] * b[(int64_t)s * ld] : 0.0;
        }
        bool hit = false;
#pragma unroll
        for (int q = 0; q < kWalk; ++q) {
            pre += w[q];
            if (!hit && s0 + q <= R && pre >= target) { hit = true; got = s0 + q; }
        }
        if (hit) break;
    }
    *out = got;
}

// An interior node v of the units of category k: j = 0..M over P_v[i][j] B_v[j] with i the parent's size, total F_v[i]
__global__ __launch_bounds__(256) void history_node_kernel(const Units un, int k, int v, int parent, const double* __restrict__ Pt, int ldp,
                                                           const double* __restrict__ B, const double* __restrict__ F, int64_t ld, int M) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= un.n_units) return;
    const int cat = un.cat[unit];
    int32_t* out = un.sizes + (int64_t)v * un.n_units + unit;
    if (cat < 0) { *out = -1; return; }
    if (cat != k) return;
    const int i = un.sizes[(int64_t)parent * un.n_units + unit];
    if (i == 0) { *out = 0; return; }                        // row 0 of P is e_0: an extinct lineage stays extinct
    const int64_t fi = unit / un.n_draws;
    const int d = un.d0 + (int)(unit - fi * un.n_draws);
    const int col = un.column[fi];
    const double target = uniform01(un.family[fi], v, 2u * (uint32_t)d, un.k0, un.k1) * F[(int64_t)i * ld + col];
    const double* p = Pt + (i - 1);
    const double* b = B + col;
    double pre = 0.0;
    int got = M;
    for (int j0 = 0; j0 <= M; j0 += kWalk) {
        double w[kWalk];
#pragma unroll
        for (int q = 0; q < kWalk; ++q) {
            const int j = j0 + q;
            w[q] = j <= M ? p[(int64_t)j * ldp] * b[(int64_t)j * ld] : 0.0;
        }
        bool hit = false;
#pragma unroll
        for (int q = 0; q < kWalk; ++q) {
            pre += w[q];
            if (!hit && j0 + q <= M && pre >= target) { hit = true; got = j0 + q; }
        }
        if (hit) break;
    }
    *out = got;
}

// A leaf v of the units of category k: its observed count, or the first tap over err[x][t] P_v[i][c] (row-major matrix)
__global__ __launch_bounds__(256) void history_leaf_kernel(const Units un, int k, int v, int parent, const double* __restrict__ P, int ldp,
                                                           const int32_t* __restrict__ cnt, const double* __restrict__ err, int n_dev, int M) {
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (unit >= un.n_units) return;
    const int cat = un.cat[unit];
    int32_t* out = un.sizes + (int64_t)v * un.n_units + unit;
    if (cat < 0) { *out = -1; return; }
    if (cat != k) return;
    const int64_t fi = unit / un.n_draws;
    const int x = cnt[un.column[fi]];
    if (err == nullptr) { *out = x; return; }
    const int i = un.sizes[(int64_t)parent * un.n_units + unit];
    const int d = un.d0 + (int)(unit - fi * un.n_draws);
    const int half = (n_dev - 1) / 2;
    const double* row = P + (int64_t)i * ldp;
    const double* e = err + (int64_t)x * n_dev;
    double total = 0.0;
    for (int t = 0; t < n_dev; ++t) {
        const int c = x - half + t;
        if (c >= 0 && c <= M) total += e[t] * row[c];
    }
    const double target = uniform01(un.family[fi], v, 2u * (uint32_t)d, un.k0, un.k1) * total;
    double pre = 0.0;
    int got = -1, last = x;
    for (int t = 0; t < n_dev; ++t) {
        const int c = x - half + t;
        if (c < 0 || c > M) continue;
        pre += e[t] * row[c];
        last = c;
        if (pre >= target) { got = c; break; }
    }
    *out = got < 0 ? last : got;
}

// The three counts of node v (grid.x), 64 draws (grid.y) and a slab of the batch's families (grid.z): every wave walks its
// share of the slab with one draw per lane, the block adds its four waves in LDS and issues one atomic per draw and count.
// Integer sums: exact in any order.
__global__ __launch_bounds__(256) void history_count_kernel(const Units un, const int32_t* __restrict__ parent_of, int n_nodes, int64_t n_fam, int64_t slab,
                                                            unsigned long long* __restrict__ n_inc, unsigned long long* __restrict__ n_dec,
                                                            unsigned long long* __restrict__ net) {
    __shared__ long long red[3][4][64];
    const int v = blockIdx.x, p = parent_of[v];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dl = blockIdx.y * 64 + lane;
    long long inc = 0, dec = 0, sum = 0;
    if (p >= 0 && dl < un.n_draws) {
        const int64_t f_begin = (int64_t)blockIdx.z * slab, f_end = min(n_fam, f_begin + slab);
        const int32_t* xv = un.sizes + (int64_t)v * un.n_units + dl;
        const int32_t* xp = un.sizes + (int64_t)p * un.n_units + dl;
        for (int64_t fi = f_begin + wave; fi < f_end; fi += 4) {
            const int a = xv[fi * un.n_draws], b = xp[fi * un.n_draws];
            if (a < 0) continue;                             // a failed family
            inc += a > b;
            dec += a < b;
            sum += a - b;
        }
    }
    red[0][wave][lane] = inc; red[1][wave][lane] = dec; red[2][wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && p >= 0 && dl < un.n_draws) {
        for (int w = 1; w < 4; ++w) { inc += red[0][w][lane]; dec += red[1][w][lane]; sum += red[2][w][lane]; }
        const int64_t o = (int64_t)(un.d0 + dl) * n_nodes + v;
        if (inc) atomicAdd(n_inc + o, (unsigned long long)inc);
        if (dec) atomicAdd(n_dec + o, (unsigned long long)dec);
        if (sum) atomicAdd(net + o, (unsigned long long)sum);      // two's complement: the sum of the differences
    }
}

// sizes [node][unit] -> out[dl][fi][node], through an LDS tile so that both sides move whole rows
__global__ __launch_bounds__(256) void history_transpose_kernel(const Units un, int n_nodes, int64_t n_fam, int32_t* __restrict__ out) {
    __shared__ int32_t tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int64_t u0 = (int64_t)blockIdx.x * 32;
    const int v0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8) {
        const int v = v0 + r;
        const int64_t unit = u0 + tx;
        tile[r][tx] = (v < n_nodes && unit < un.n_units) ? un.sizes[(int64_t)v * un.n_units + unit] : 0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t unit = u0 + r;
        const int v = v0 + tx;
        if (unit >= un.n_units || v >= n_nodes) continue;
        const int64_t fi = unit / un.n_draws;
        const int64_t dl = unit - fi * un.n_draws;
        out[(dl * n_fam + fi) * n_nodes + v] = tile[tx][r];
    }
}

}  // namespace

int history_impl(cafe_ctx* c, const cafe_params* pr, int32_t n_draws, uint64_t seed, const cafe_history_out* out) {
    if (const int rc = check_call_args(c, "cafe_sample_histories", pr, out)) return rc;
    if (n_draws < 1 || n_draws > 65536) { set_err(c, "cafe_sample_histories: n_draws must lie in 1..65536"); return CAFE_ERR_ARGUMENT; }
    if (const int rc = check_model_args(c, "cafe_sample_histories", pr)) return rc;
    PosteriorCall pc;
    if (const int rc = open_posterior_call(c, pr, &pc)) return rc;
    hipStream_t s = pc.s;
    UpPanels& up = pc.up;
    const int M = c->M, R = c->R, n = c->n_nodes, rows = c->N, K = pc.K, nI = pc.nI, n_dev = pc.n_dev;
    const bool want_sizes = out->sizes != nullptr, want_counts = out->n_increase || out->n_decrease || out->net_change;

    // What does not depend on the batches comes off the budget first: the three count arrays of all draws, the prior, the
    // category weights, the error model and the parents.  Of the rest three quarters hold B and F of every interior node
    // (one category at a time) and Z_k of a column batch, the last quarter the batch's family and column lists and the units
    // of a pass over the draws: a size per node, the category and, when the sizes are asked for, their transposed copy.
    // One draw per pass is the least.
    size_t budget = 0;
    if (const int rc = panel_budget(c, &budget)) return rc;
    const size_t count_len = (size_t)n_draws * n;
    const size_t fixed = sizeof(unsigned long long) * 3 * count_len + sizeof(double) * ((size_t)R + K + (pc.has_err ? (size_t)(M + 1) * n_dev : 0)) + sizeof(int32_t) * n;
    if (fixed >= budget) {
        set_err(c, "cafe_sample_histories: %zu bytes of workspace cannot hold the counts of %d draws", budget, (int)n_draws);
        return CAFE_ERR_MEMORY;
    }
    budget -= fixed;
    const size_t per_col = ((size_t)2 * nI * rows + K + 1) * sizeof(double);
    const int64_t cols = std::min<int64_t>(c->Fp, (int64_t)((budget - budget / 4) / per_col) / kBN * kBN);
    if (cols < kBN) {
        set_err(c, "cafe_sample_histories: not enough device memory for the panels of %d interior nodes", nI);
        return CAFE_ERR_MEMORY;
    }
    // families per column batch (a column's duplicates come with it)
    std::vector<int64_t> batch_fams((size_t)((c->Fp + cols - 1) / cols), 0);
    for (int64_t f = 0; f < c->F_all; ++f) ++batch_fams[(size_t)(c->ref_of[f] / cols)];
    int64_t max_fams = 1;
    for (int64_t b : batch_fams) max_fams = std::max(max_fams, b);
    const size_t per_unit = ((size_t)n * (want_sizes ? 2 : 1) + 1) * sizeof(int32_t);
    const size_t lists = (sizeof(int64_t) + sizeof(int32_t)) * (size_t)max_fams;
    int64_t pass_draws = budget / 4 > lists ? (int64_t)((budget / 4 - lists) / per_unit) / max_fams : 0;
    pass_draws = std::max<int64_t>(1, std::min<int64_t>({pass_draws, (int64_t)n_draws, ((int64_t)1 << 30) / max_fams}));
    if (max_fams * pass_draws > ((int64_t)1 << 31) - 256) { set_err(c, "cafe_sample_histories: too many families share one column batch"); return CAFE_ERR_MEMORY; }
    const int64_t max_units = max_fams * pass_draws;
    c->history_batches = (int)batch_fams.size();
    c->history_passes = (int)((n_draws + pass_draws - 1) / pass_draws);

    DevBuf wd, wz, dfam, dcol, dcat, dsz, dtr, dcnt, dpar;
    if (hipMalloc(&wd.p, (size_t)2 * nI * rows * cols * sizeof(double)) != hipSuccess || hipMalloc(&wz.p, (size_t)(K + 1) * cols * sizeof(double)) != hipSuccess ||
        alloc_constants(c, kNoPriorLogs, &pc) != hipSuccess || hipMalloc(&dfam.p, sizeof(int64_t) * max_fams) != hipSuccess || hipMalloc(&dcol.p, sizeof(int32_t) * max_fams) != hipSuccess ||
        hipMalloc(&dcat.p, sizeof(int32_t) * max_units) != hipSuccess || hipMalloc(&dsz.p, sizeof(int32_t) * (size_t)n * max_units) != hipSuccess ||
        (want_sizes && hipMalloc(&dtr.p, sizeof(int32_t) * (size_t)n * max_units) != hipSuccess) ||
        hipMalloc(&dcnt.p, sizeof(unsigned long long) * 3 * count_len) != hipSuccess || hipMalloc(&dpar.p, sizeof(int32_t) * n) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "cafe_sample_histories: cannot allocate the workspace (%lld columns, %lld draws per pass)", (long long)cols, (long long)pass_draws);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemsetAsync(wd.p, 0, (size_t)2 * nI * rows * cols * sizeof(double), s));
    HIP_TRY(c, hipMemsetAsync(dcnt.p, 0, sizeof(unsigned long long) * 3 * count_len, s));
    const int64_t pstride = (int64_t)rows * cols;
    up.place(wd.p, nI, pstride);
    double* d_Zk = static_cast<double*>(wz.p);               // [K][cols]
    double* d_Z = d_Zk + (int64_t)K * cols;
    unsigned long long* d_inc = static_cast<unsigned long long*>(dcnt.p);
    unsigned long long *d_dec = d_inc + count_len, *d_net = d_dec + count_len;
    const std::vector<int32_t> par(c->parent.begin(), c->parent.end());
    HIP_TRY(c, hipMemcpyAsync(dpar.p, par.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    if (const int rc = upload_constants(c, pr, &pc)) return rc;      // its synchronise covers the parents' copy

    std::vector<double> h_Z(cols);
    std::vector<int64_t> fams;
    std::vector<int32_t> fcols, h_cat, h_sizes;
    const int root = c->root;

    for (int64_t f0 = 0; f0 < c->Fp; f0 += cols) {
        const int64_t ld = std::min<int64_t>(cols, c->Fp - f0);
        const unsigned gb = (unsigned)((ld + 255) / 256);
        fams.clear(); fcols.clear();
        for_each_family_of_chunk(c, f0, ld, [&](int64_t f, int64_t col) { fams.push_back(f); fcols.push_back((int32_t)col); });
        const int64_t nb = (int64_t)fams.size();
        // ---- every Z_k; afterwards the panels hold category K - 1
        int held = -1;
        for (int k = 0; k < K; ++k) {
            if (const int rc = marginal_up_pass(c, up, k, f0, ld, s, pc.timer)) return rc;
            held = k;
            CAFE_LAUNCH(c, history_rootz_kernel, dim3(gb), dim3(256), 0, s, up.panel(up.B, root), pc.prior, R, ld, d_Zk + (int64_t)k * cols);
        }
        CAFE_LAUNCH(c, history_z_kernel, dim3(gb), dim3(256), 0, s, d_Zk, pc.probs, K, cols, ld, d_Z);
        HIP_TRY(c, hipMemcpyAsync(h_Z.data(), d_Z, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for (int64_t i = 0; i < nb; ++i) {
            const double z = h_Z[fcols[i]];
            const bool bad = evidence_failed(z);
            if (out->log_evidence) out->log_evidence[fams[i]] = bad ? kNaN : std::log(z);
            if (out->failed) out->failed[fams[i]] = bad ? 1 : 0;
        }
        if (nb == 0 || !(want_sizes || want_counts || out->category)) continue;
        HIP_TRY(c, hipMemcpyAsync(dfam.p, fams.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(dcol.p, fcols.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice, s));
        // ---- the draws, in passes of pass_draws; a pass sweeps the categories downwards, so the first
        // pass starts on the panels that the Z_k sweep left
        for (int d0 = 0; d0 < n_draws; d0 += (int)pass_draws) {
            Units un{};
            un.family = static_cast<const int64_t*>(dfam.p);
            un.column = static_cast<const int32_t*>(dcol.p);
            un.n_draws = (int)std::min<int64_t>(pass_draws, n_draws - d0);
            un.d0 = d0;
            un.n_units = nb * un.n_draws;
            un.k0 = (uint32_t)seed; un.k1 = (uint32_t)(seed >> 32);
            un.cat = static_cast<int32_t*>(dcat.p);
            un.sizes = static_cast<int32_t*>(dsz.p);
            const unsigned ub = (unsigned)((un.n_units + 255) / 256);
            CAFE_LAUNCH(c, history_category_kernel, dim3(ub), dim3(256), 0, s, un, d_Zk, pc.probs, K, cols, root);
            for (int k = K - 1; k >= 0; --k) {
                if (k != held) {
                    if (const int rc = marginal_up_pass(c, up, k, f0, ld, s, pc.timer)) return rc;
                    held = k;
                }
                CAFE_LAUNCH(c, history_root_kernel, dim3(ub), dim3(256), 0, s, un, k, up.panel(up.B, root), pc.prior, R, ld, d_Zk + (int64_t)k * cols, root);
                for (int v = n - 1; v >= 0; --v) {           // parents before children
                    if (v == root) continue;
                    const int p = c->parent[v];
                    if (c->leaf_taxon[v] >= 0)
                        CAFE_LAUNCH(c, history_leaf_kernel, dim3(ub), dim3(256), 0, s, un, k, v, p, leaf_matrix(c, v, k), c->pool.ld, leaf_counts(c, v, f0), up.err,
                                    n_dev, M);
                    else
                        CAFE_LAUNCH(c, history_node_kernel, dim3(ub), dim3(256), 0, s, un, k, v, p, interior_matrix(c, v, k), c->kpool.ld, up.panel(up.B, v),
                                    up.panel(up.F, v), ld, M);
                }
            }
            if (want_counts) {
                const int64_t slab = std::max<int64_t>(256, (nb + 63) / 64);
                CAFE_LAUNCH(c, history_count_kernel, dim3((unsigned)n, (unsigned)((un.n_draws + 63) / 64), (unsigned)((nb + slab - 1) / slab)), dim3(256), 0, s, un,
                            static_cast<const int32_t*>(dpar.p), n, nb, slab, d_inc, d_dec, d_net);
            }
            if (out->category) {
                h_cat.resize((size_t)un.n_units);
                HIP_TRY(c, hipMemcpyAsync(h_cat.data(), un.cat, sizeof(int32_t) * (size_t)un.n_units, hipMemcpyDeviceToHost, s));
            }
            if (want_sizes) {
                h_sizes.resize((size_t)un.n_units * n);
                CAFE_LAUNCH(c, history_transpose_kernel, dim3((unsigned)((un.n_units + 31) / 32), (unsigned)((n + 31) / 32)), dim3(256), 0, s, un, n, nb,
                            static_cast<int32_t*>(dtr.p));
                HIP_TRY(c, hipMemcpyAsync(h_sizes.data(), dtr.p, sizeof(int32_t) * (size_t)un.n_units * n, hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(c, hipStreamSynchronize(s));
            for (int dl = 0; dl < un.n_draws; ++dl)
                for (int64_t i = 0; i < nb; ++i) {
                    const size_t dst = (size_t)(d0 + dl) * c->F_all + fams[i];
                    if (out->category) out->category[dst] = h_cat[(size_t)i * un.n_draws + dl];
                    if (want_sizes) std::copy_n(h_sizes.data() + ((size_t)dl * nb + i) * n, n, out->sizes + dst * n);
                }
        }
    }
    if (want_counts) {
        int64_t* dst[3] = {out->n_increase, out->n_decrease, out->net_change};
        for (int a = 0; a < 3; ++a)
            if (dst[a]) HIP_TRY(c, hipMemcpyAsync(dst[a], d_inc + a * count_len, sizeof(int64_t) * count_len, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    close_posterior_call(c, nullptr);                        // no timer: cafe_debug_marginal_gemm keeps its figures
    return CAFE_OK;
}

}  // namespace cafe

extern "C" {

int cafe_sample_histories(cafe_ctx* ctx, const cafe_params* params, int32_t n_draws, uint64_t seed, const cafe_history_out* out) {
    return cafe::guarded_observed(ctx, "cafe_sample_histories", [&] { return cafe::history_impl(ctx, params, n_draws, seed, out); });
}

int cafe_debug_history_batches(cafe_ctx* ctx, int32_t* column_batches, int32_t* draw_passes) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (column_batches) *column_batches = ctx->history_batches;
    if (draw_passes) *draw_passes = ctx->history_passes;
    return CAFE_OK;
}

}
