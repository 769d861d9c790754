// cafe_score_gain: the gain model (family_gain.hip) under ONE set of rates for the whole list, on a dense prune.
// cafe_score_per_family_gain re-runs the O(N^2) row recurrence of a branch for every (family, branch); with shared rates the
// matrix of a branch is the same for every family, so this entry builds each distinct matrix once and prunes all listed
// families together, one panel column per list entry:
//
//   build    one wave per distinct key (lambda index, quantized t): the per-family kernel's recurrence -- gain_row0, then
//            bd_row_step -- whose rows are STORED.  Both readers want column c of P contiguous in the parent size s (k-major,
//            Pt[c][s] = P[s][c]), so the wave parks T rows in LDS and then writes, per column, the T consecutive sizes.
//            Row 0 and column 0 are a row and a column like any other.  A saturated key stores row 0 and zeros below it.
//   product  per tree level, every node p of the level at once (a device op table):
//            B_p[s][f] = prod_{interior children} F_c[s][f] * prod_{leaf children} sum_taps err * P_c[s][count_f + tap]
//   gemm     per tree level, every interior non-root node v of the level at once: F_v = P_v B_v with v_mfma_f64_16x16x4_f64,
//            64 x 128 x 16 tiles, A and B staged through two LDS buffers, every load guarded by the order
//   root     lnL_f from mass[j] B_root[j][f], j = 0..R, in logarithms, the maximum or the sum by the context's root rule
//
// Plain fp64, no rescaling.  A column's value is computed by the same operations in the same order wherever the column
// stands, so it depends on the family's counts and the rates only: not on its position, not on the batch cut.
#include <map>
#include <utility>

#include "family_frame.h"
#include "family_gain_kernel.h"

namespace cafe {
namespace {

constexpr int kGdCols = 128;         // column tile: batches are whole tiles

// ---------------------------------------------------------------------------------------------------------------- build
struct GainBuildArgs {
    const SlotParamGain* slots;      // [keys]
    double* Pt;                      // [keys][N][ldp]
    int32_t N, ldp;
    int64_t stride;                  // doubles per matrix
};

// rows parked before they are turned: 64 KB of LDS at most (a row is 64 E doubles)
template <int E>
constexpr int gain_turn_rows() { return 128 / E < 16 ? 128 / E : 16; }

template <int E>
__global__ __launch_bounds__(64) void gain_dense_build_kernel(const GainBuildArgs a) {
    constexpr int T = gain_turn_rows<E>(), W = 64 * E;
    __shared__ double turn[T * W];
    const int lane = threadIdx.x, c0 = lane * E, N = a.N;
    const SlotParamGain sp = a.slots[blockIdx.x];
    double* __restrict__ Pt = a.Pt + (int64_t)blockIdx.x * a.stride;

    double p[E];                                       // P[row][c0 + i]; the columns past the matrix are never stored
    gain_row0<E>(sp, c0, p);
    const int n_run = sp.zero ? 1 : N;                 // saturated / degenerate: row 0 alone is run
    BdRowConsts<E, true> rc;
    rc.init(sp.alpha, sp.beta, sp.q, lane);
    for (int r = 0; r < n_run; ++r) {
        if (r > 0) bd_row_step<E, false>(rc, nullptr, 0.0, lane, p);
        const int t = r % T;
#pragma unroll
        for (int i = 0; i < E; ++i) turn[t * W + c0 + i] = p[i];
        if (t == T - 1 || r == n_run - 1) {
            __syncthreads();                           // one wave per block: orders the LDS writes before the turned reads
            const int r0 = r - t;
            for (int c = lane; c < N; c += 64) {
                double* __restrict__ dst = Pt + (int64_t)c * a.ldp + r0;
                for (int k = 0; k <= t; ++k) dst[k] = turn[k * W + c];
            }
            __syncthreads();                           // the rows are read before the next ones overwrite them
        }
    }
    if (sp.zero)
        for (int c = lane; c < N; c += 64)
            for (int s = 1; s < N; ++s) Pt[(int64_t)c * a.ldp + s] = 0.0;
}

hipError_t launch_build(const GainBuildArgs& a, int n_keys, hipStream_t s) {
    if (a.N > bd_matrix_max_order() || a.N > a.ldp) return hipErrorInvalidValue;
    return for_lane_width(a.N, [&](auto e) {
        (void)hipGetLastError();
        hipLaunchKernelGGL((gain_dense_build_kernel<decltype(e)::value>), dim3((unsigned)n_keys), dim3(64), 0, s, a);
        return hipGetLastError();
    });
}

// ---------------------------------------------------------------------------------------------------------------- product
struct GainChild {
    int64_t src;                     // interior child: its F panel (doubles from `panels`); leaf: its matrix (doubles from `mats`)
    int32_t taxon;                   // row of `counts` for a leaf, -1 for an interior child
    int32_t pad;
};
struct GainProdOp {
    int64_t dst;                     // B panel of the node
    int32_t rows;                    // sizes 0..rows-1
    int32_t child0, n_children;      // children[child0 .. child0 + n_children)
    int32_t pad;
};
struct GainProdArgs {
    const GainProdOp* ops;
    const GainChild* children;
    double* panels;
    const double* mats;
    const int64_t* col;              // [ld] the entry's column in `counts`, -1: every count 0
    const int32_t* counts;
    int64_t counts_ld, ld, ncols;    // ld: columns of a panel; ncols: those of this batch (col[] is filled that far)
    const double* err;               // [(M+1)][n_dev] or nullptr
    int32_t n_dev, M, ldp;
};

constexpr int kGdProdRows = 16;

// grid (column blocks of 256, row blocks of 16, nodes of the level); a thread owns one column and 16 sizes
__global__ __launch_bounds__(256) void gain_dense_product_kernel(const GainProdArgs a) {
    const GainProdOp op = a.ops[blockIdx.z];
    const int i0 = blockIdx.y * kGdProdRows;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 >= op.rows || f >= a.ncols) return;
    const int n = min(kGdProdRows, op.rows - i0);
    const int64_t col = a.col[f];
    double v[kGdProdRows];
#pragma unroll
    for (int j = 0; j < kGdProdRows; ++j) v[j] = 1.0;
    for (int k = 0; k < op.n_children; ++k) {
        const GainChild ch = a.children[op.child0 + k];
        if (ch.taxon < 0) {
            const double* __restrict__ F = a.panels + ch.src + (int64_t)i0 * a.ld + f;
#pragma unroll
            for (int j = 0; j < kGdProdRows; ++j)
                if (j < n) v[j] *= F[(int64_t)j * a.ld];
            continue;
        }
        const int x = col >= 0 ? a.counts[(int64_t)ch.taxon * a.counts_ld + col] : 0;
        if (count_is_missing(x)) continue;             // a missing cell: the factor is exactly 1.0 for every parent size
        const double* __restrict__ P = a.mats + ch.src + i0;
        if (a.err == nullptr) {
            const bool in = x <= a.M;                  // (a count past the matrix has no column: likelihood 0)
            const double* __restrict__ pc = P + (int64_t)(in ? x : 0) * a.ldp;
#pragma unroll
            for (int j = 0; j < kGdProdRows; ++j)
                if (j < n) v[j] *= in ? pc[j] : 0.0;
        } else {
            const int lo = x - (a.n_dev - 1) / 2;      // taps outside [0, M] are dropped
            double fac[kGdProdRows];
#pragma unroll
            for (int j = 0; j < kGdProdRows; ++j) fac[j] = 0.0;
            for (int t = 0; t < a.n_dev; ++t) {
                const int c = lo + t;
                if (c < 0 || c > a.M || x > a.M) continue;
                const double w = a.err[(int64_t)x * a.n_dev + t];
                const double* __restrict__ pc = P + (int64_t)c * a.ldp;
#pragma unroll
                for (int j = 0; j < kGdProdRows; ++j)
                    if (j < n) fac[j] = fma(pc[j], w, fac[j]);
            }
#pragma unroll
            for (int j = 0; j < kGdProdRows; ++j) v[j] *= fac[j];
        }
    }
    double* __restrict__ dst = a.panels + op.dst + (int64_t)i0 * a.ld + f;
#pragma unroll
    for (int j = 0; j < kGdProdRows; ++j)
        if (j < n) dst[(int64_t)j * a.ld] = v[j];
}

// ---------------------------------------------------------------------------------------------------------------- GEMM
// Block tile 64 sizes x 128 columns, K step 16; wave w owns the 32 columns 32 w .. over all 64 rows: 4 x 2 accumulator tiles of
// v_mfma_f64_16x16x4_f64 (A fragment: row = lane & 15, k = lane >> 4; B fragment: k = lane >> 4, column = lane & 15; D: row =
// (lane >> 4) + 4 * register, column = lane & 15) -- the tile of sum_product.hip.  Both tiles stand in LDS k-major with a
// 16-double pad, TWICE: while the MFMAs read one pair of buffers the next K step's global loads land in registers and are
// stored into the other pair, so a K step costs one barrier.  2 x 16 x (80 + 144) doubles = 57344 bytes of LDS.
constexpr int kGdMT = 64, kGdKT = 16;
constexpr int kGdLdA = kGdMT + 16, kGdLdX = kGdCols + 16;

struct GainGemmOp {
    int64_t Pt, B, F;                // matrix (doubles from `mats`), panels (doubles from `panels`)
    int32_t nr;                      // rows s = 0..nr-1 of F
    int32_t pad;
};
struct GainGemmArgs {
    const GainGemmOp* ops;
    const double* mats;
    double* panels;
    int64_t ld;
    int32_t nk, ldp;                 // contraction over c = 0..nk-1
};

// grid (column tiles, row tiles of the tallest op, interior non-root nodes of the level)
__global__ __launch_bounds__(256) void gain_dense_gemm_kernel(const GainGemmArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][kGdKT * kGdLdA];
    __shared__ __attribute__((aligned(16))) double Xs[2][kGdKT * kGdLdX];
    const GainGemmOp op = a.ops[blockIdx.z];
    const int r0 = blockIdx.y * kGdMT;
    if (r0 >= op.nr) return;                           // (block-uniform, ahead of every barrier)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * kGdCols, ld = a.ld;
    const int nr = op.nr, nk = a.nk, ldp = a.ldp;
    const double* __restrict__ Pt = a.mats + op.Pt;
    const double* __restrict__ X = a.panels + op.B;
    typedef double d4 __attribute__((ext_vector_type(4)));
    d4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
    double ra[4];
    double2 rx[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + lane, k = k0 + wave + 4 * u;                 // A[r][k] = Pt[k][r]: 64 consecutive sizes per k
            ra[u] = (r < nr && k < nk) ? Pt[(int64_t)k * ldp + r] : 0.0;
            rx[u] = k < nk ? *reinterpret_cast<const double2*>(X + (int64_t)k * ld + c0 + 2 * lane) : make_double2(0.0, 0.0);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            As[buf][(wave + 4 * u) * kGdLdA + lane] = ra[u];
            *reinterpret_cast<double2*>(&Xs[buf][(wave + 4 * u) * kGdLdX + 2 * lane]) = rx[u];
        }
    };
    load(0);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < nk; k0 += kGdKT, buf ^= 1) {
        const bool more = k0 + kGdKT < nk;
        if (more) load(k0 + kGdKT);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            double af[4], bf[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = As[buf][(4 * s4 + l4) * kGdLdA + 16 * i + l15];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Xs[buf][(4 * s4 + l4) * kGdLdX + 32 * wave + 16 * j + l15];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (more) stage(buf ^ 1);                      // the other pair: its readers passed the barrier of the step before
        __syncthreads();
    }
    double* __restrict__ F = a.panels + op.F;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 16 * i + l4 + 4 * q;
                if (r < nr) F[(int64_t)r * ld + c0 + 32 * wave + 16 * j + l15] = acc[i][j][q];
            }
}

// ---------------------------------------------------------------------------------------------------------------- root
struct GainRootArgs {
    const double* B;                 // the root's panel
    const double* logmass;           // [R + 1] log(root_absent), log1p(-root_absent) + log (double)(float)prior_j
    double* out;                     // [ld]
    int64_t ld;
    int32_t R, sum_rule;
};

// 64 columns per block, the sizes dealt to four waves: t_j = log B[j][f] + logmass[j], then the maximum, or m + log sum exp(t - m)
__global__ __launch_bounds__(256) void gain_dense_root_kernel(const GainRootArgs a) {
    __shared__ double red[4][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 64 + x;    // (ld is a multiple of 128)
    const double ninf = -__builtin_huge_val();
    double m = ninf;
    for (int j = y; j <= a.R; j += 4) {
        const double t = log(a.B[(int64_t)j * a.ld + f]) + a.logmass[j];
        if (t > m) m = t;
    }
    red[y][x] = m;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) m = red[k][x] > m ? red[k][x] : m;
    __syncthreads();
    double s = 0.0;
    if (a.sum_rule)
        for (int j = y; j <= a.R; j += 4) {
            const double t = log(a.B[(int64_t)j * a.ld + f]) + a.logmass[j];
            s += t == ninf ? 0.0 : exp(t - m);
        }
    red[y][x] = s;
    __syncthreads();
    if (y == 0) a.out[f] = a.sum_rule ? m + log((red[0][x] + red[1][x]) + (red[2][x] + red[3][x])) : m;
}

// ---------------------------------------------------------------------------------------------------------------- host
enum { kGdBuild = 0, kGdProduct = 1, kGdGemm = 2, kGdRoot = 3 };

// HIP events around the launches of a call, by kind (cafe_set_profiling)
struct GainTimer {
    bool on = false;
    std::vector<std::pair<int, hipEvent_t>> ev;
    ~GainTimer() { for (auto& e : ev) (void)hipEventDestroy(e.second); }
    void mark(int kind, hipStream_t s) {
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
        ev.push_back({kind, e});
        (void)hipEventRecord(e, s);
    }
    void collect(double ms[4]) const {
        for (size_t i = 0; on && i + 1 < ev.size(); i += 2) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, ev[i].second, ev[i + 1].second) == hipSuccess) ms[ev[i].first] += t;
        }
    }
};

template <class T>
size_t put(std::vector<char>& blob, const std::vector<T>& v) {
    const size_t at = family_align_up(blob.size());
    blob.resize(at + sizeof(T) * v.size());
    if (!v.empty()) std::memcpy(blob.data() + at, v.data(), sizeof(T) * v.size());
    return at;
}

int score_gain_impl(cafe_ctx* c, const cafe_params* pr, const double* lam, const double* mus, const double* nus, double root_absent, int64_t n,
                    const int64_t* family, double* family_lnl) {
    const char* const who = "cafe_score_gain";
    if (!pr || !pr->prior) { set_err(c, "%s: params with a prior are required", who); return CAFE_ERR_ARGUMENT; }
    if (pr->model != CAFE_MODEL_BASE) { set_err(c, "%s: base model only", who); return CAFE_ERR_ARGUMENT; }
    if (c->comm) { set_err(c, "%s: not valid on a context with a communicator attached", who); return CAFE_ERR_STATE; }
    if (n < 0 || !lam || (n > 0 && (!family || !family_lnl))) { set_err(c, "%s: lambdas, family and family_lnl are required", who); return CAFE_ERR_ARGUMENT; }
    if ((c->n_dev > 0) != (pr->error_model != nullptr)) {
        set_err(c, "%s: error model %s but the problem was created with n_deviations=%d", who, pr->error_model ? "given" : "missing", c->n_dev);
        return CAFE_ERR_ARGUMENT;
    }
    if (!c->device_ready || !c->d_counts) { set_err(c, "%s: the context holds no family table", who); return CAFE_ERR_STATE; }
    for (int64_t i = 0; i < n; ++i)
        if (family[i] < -1 || family[i] >= c->F_all) {
            set_err(c, "%s: family index %lld outside -1..%lld", who, (long long)family[i], (long long)c->F_all - 1);
            return CAFE_ERR_ARGUMENT;
        }
    if (const int rc = gain_rates_check(c, who, 1, nus, root_absent)) return rc;
    if (n == 0) return CAFE_OK;
    const int nn = c->n_nodes, L = c->n_lambdas, N = c->N, M = c->M, R = c->R, ldp = round_up(N, 2);

    // ---- what the host decides alone: an invalid rate set is -inf in every entry, a NaN lambda that passes the rule NaN
    c->last.state = LastCall::kNone;                   // cafe_family_results is not meaningful after this call
    for (int k = 0; k < 4; ++k) c->gain_dense_ms[k] = 0.0;
    c->gain_dense_flops = 0.0;
    {
        bool nan = false;
        for (int k = 0; k < L; ++k) nan = nan || std::isnan(lam[k]);
        const bool valid = lambdas_valid(c, lam) && death_rates_ok(L, mus);
        if (!valid || nan) {
            std::fill(family_lnl, family_lnl + n, valid ? std::numeric_limits<double>::quiet_NaN() : -std::numeric_limits<double>::infinity());
            return CAFE_OK;
        }
    }

    // ---- keys, levels and the op tables.  A node's height: 0 when its children are leaves, else 1 + its tallest interior child's;
    // a level's product reads the F panels of the levels below it, its GEMMs read the level's own B panels
    std::map<std::pair<int, long>, int> key_of;
    std::vector<SlotParamGain> slots;
    std::vector<int> node_key(nn, -1), height(nn, -1), bidx(nn, -1), fidx(nn, -1);
    int n_pan = 0, n_levels = 0;
    for (int u = 0; u < nn; ++u) {
        if (u != c->root) {
            const auto it = key_of.emplace(std::make_pair(c->lam_idx[u], quantize_time(c->blen[u])), (int)slots.size());
            if (it.second) slots.push_back(gain_branch_slot(c, u, lam, mus, nus));
            node_key[u] = it.first->second;
        }
        if (c->leaf_taxon[u] >= 0) continue;
        height[u] = 0;
        for (int ch : c->children[u]) height[u] = std::max(height[u], height[ch] + 1);
        n_levels = std::max(n_levels, height[u] + 1);
        bidx[u] = n_pan++;
        if (u != c->root) fidx[u] = n_pan++;
    }
    if (c->leaf_taxon[c->root] >= 0 || height[c->root] != n_levels - 1) { set_err(c, "%s: the root is not the tallest node of the tree", who); return CAFE_ERR_STATE; }
    const int n_keys = (int)slots.size();
    const int64_t mat_stride = (int64_t)N * ldp;

    // ---- columns per batch: the matrices stand once, a batch adds its panels
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t fixed_bytes = sizeof(double) * (size_t)mat_stride * n_keys + ((size_t)64 << 10) + sizeof(GainChild) * (size_t)nn +
                               sizeof(GainProdOp) * (size_t)nn + sizeof(GainGemmOp) * (size_t)nn + sizeof(SlotParamGain) * (size_t)n_keys +
                               sizeof(double) * ((size_t)R + 1 + (size_t)(M + 1) * c->n_dev);
    const size_t column_bytes = sizeof(double) * (size_t)n_pan * N + sizeof(int64_t) + sizeof(double);
    size_t budget = 0;
    HIP_TRY(c, workspace_budget(c->workspace_limit, c->pf_dev_bytes, &budget));
    int64_t entries = budget > fixed_bytes ? (int64_t)((budget - fixed_bytes) / column_bytes) / kGdCols * kGdCols : 0;
    entries = std::max<int64_t>(kGdCols, std::min<int64_t>(entries, round_up64(n, kGdCols)));
    if (c->pf_max_batch > 0) entries = std::min(entries, c->pf_max_batch);
    const int64_t ld = round_up64(entries, kGdCols);
    const int64_t pan_stride = (int64_t)N * ld;

    std::vector<GainChild> children;
    std::vector<GainProdOp> prod_ops;
    std::vector<GainGemmOp> gemm_ops;
    std::vector<int> prod_off{0}, gemm_off{0}, prod_rows, gemm_rows;       // per level: its ops, its tallest op
    for (int lv = 0; lv < n_levels; ++lv) {
        int pr_rows = 0, gm_rows = 0;
        for (int u = 0; u < nn; ++u) {
            if (height[u] != lv) continue;
            GainProdOp po{};
            po.dst = bidx[u] * pan_stride;
            po.rows = (u == c->root ? R : M) + 1;
            po.child0 = (int32_t)children.size();
            for (int ch : c->children[u]) {
                const bool leaf = c->leaf_taxon[ch] >= 0;
                children.push_back({leaf ? node_key[ch] * mat_stride : fidx[ch] * pan_stride, leaf ? c->leaf_taxon[ch] : -1, 0});
            }
            po.n_children = (int32_t)children.size() - po.child0;
            prod_ops.push_back(po);
            pr_rows = std::max(pr_rows, po.rows);
            if (u == c->root) continue;
            const int nr = (c->parent[u] == c->root ? R : M) + 1;
            gemm_ops.push_back({node_key[u] * mat_stride, bidx[u] * pan_stride, fidx[u] * pan_stride, nr, 0});
            gm_rows = std::max(gm_rows, nr);
        }
        prod_off.push_back((int)prod_ops.size()); gemm_off.push_back((int)gemm_ops.size());
        prod_rows.push_back(pr_rows); gemm_rows.push_back(gm_rows);
    }
    std::vector<double> reals((size_t)R + 1 + (size_t)(M + 1) * c->n_dev);  // log mass of the root sizes, error model
    reals[0] = std::log(root_absent);
    for (int j = 0; j < R; ++j) reals[j + 1] = std::log1p(-root_absent) + std::log((double)pr->prior[j]);    // compute() returns float
    if (c->n_dev > 0) std::memcpy(reals.data() + R + 1, pr->error_model, sizeof(double) * (size_t)(M + 1) * c->n_dev);

    std::vector<char> blob;
    const size_t o_children = put(blob, children), o_prod = put(blob, prod_ops), o_gemm = put(blob, gemm_ops), o_slots = put(blob, slots),
                 o_reals = put(blob, reals);
    const size_t o_col = family_align_up(blob.size()), o_out = o_col + family_align_up(sizeof(int64_t) * ld),
                 o_mats = o_out + family_align_up(sizeof(double) * ld), o_pan = o_mats + family_align_up(sizeof(double) * (size_t)mat_stride * n_keys),
                 need = o_pan + sizeof(double) * (size_t)pan_stride * n_pan;
    if (need > c->pf_dev_bytes) {
        if (c->pf_dev) { HIP_TRY(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->pf_dev); c->pf_dev = nullptr; c->pf_dev_bytes = 0; }
        if (hipMalloc(&c->pf_dev, need) != hipSuccess) {
            (void)hipGetLastError();
            c->pf_dev = nullptr;
            set_err(c, "%s: cannot allocate a workspace of %zu bytes (%d matrices of order %d, %lld columns per batch)", who, need, n_keys, N, (long long)ld);
            return CAFE_ERR_MEMORY;
        }
        c->pf_dev_bytes = need;
    }
    char* base = static_cast<char*>(c->pf_dev);
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(base, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    GainTimer timer;
    timer.on = c->profile != 0;

    double* mats = reinterpret_cast<double*>(base + o_mats);
    double* panels = reinterpret_cast<double*>(base + o_pan);
    const double* d_reals = reinterpret_cast<const double*>(base + o_reals);
    GainBuildArgs ba{reinterpret_cast<const SlotParamGain*>(base + o_slots), mats, N, ldp, mat_stride};
    timer.mark(kGdBuild, s);
    HIP_TRY(c, launch_build(ba, n_keys, s));
    timer.mark(kGdBuild, s);

    GainProdArgs pa{};
    pa.ops = reinterpret_cast<const GainProdOp*>(base + o_prod); pa.children = reinterpret_cast<const GainChild*>(base + o_children);
    pa.panels = panels; pa.mats = mats; pa.col = reinterpret_cast<const int64_t*>(base + o_col);
    pa.counts = c->d_counts; pa.counts_ld = c->Fp; pa.ld = ld;
    pa.err = c->n_dev > 0 ? d_reals + R + 1 : nullptr;
    pa.n_dev = c->n_dev; pa.M = M; pa.ldp = ldp;
    GainGemmArgs ga{reinterpret_cast<const GainGemmOp*>(base + o_gemm), mats, panels, ld, M + 1, ldp};
    GainRootArgs ra{panels + bidx[c->root] * pan_stride, d_reals, reinterpret_cast<double*>(base + o_out), ld, R, c->root_rule == CAFE_ROOT_SUM ? 1 : 0};

    std::vector<int64_t> col((size_t)ld);
    std::vector<double> res((size_t)ld);
    for (int64_t b0 = 0; b0 < n; b0 += entries) {
        const int64_t nb = std::min(entries, n - b0), cols = round_up64(nb, kGdCols);
        for (int64_t b = 0; b < cols; ++b) col[b] = (b < nb && family[b0 + b] >= 0) ? c->ref_of[family[b0 + b]] : -1;    // (padding: the absent profile)
        HIP_TRY(c, hipMemcpyAsync(base + o_col, col.data(), sizeof(int64_t) * cols, hipMemcpyHostToDevice, s));
        const unsigned tiles = (unsigned)(cols / kGdCols);
        for (int lv = 0; lv < n_levels; ++lv) {
            const int np = prod_off[lv + 1] - prod_off[lv], ng = gemm_off[lv + 1] - gemm_off[lv];
            GainProdArgs p = pa;
            p.ops += prod_off[lv];
            p.ncols = cols;
            timer.mark(kGdProduct, s);
            CAFE_LAUNCH(c, gain_dense_product_kernel, dim3((unsigned)((cols + 255) / 256), (unsigned)((prod_rows[lv] + kGdProdRows - 1) / kGdProdRows), (unsigned)np),
                        dim3(256), 0, s, p);
            timer.mark(kGdProduct, s);
            if (ng == 0) continue;
            GainGemmArgs g = ga;
            g.ops += gemm_off[lv];
            timer.mark(kGdGemm, s);
            CAFE_LAUNCH(c, gain_dense_gemm_kernel, dim3(tiles, (unsigned)((gemm_rows[lv] + kGdMT - 1) / kGdMT), (unsigned)ng), dim3(256), 0, s, g);
            timer.mark(kGdGemm, s);
            for (int k = gemm_off[lv]; k < gemm_off[lv + 1]; ++k)
                c->gain_dense_flops += 2.0 * round_up(gemm_ops[k].nr, kGdMT) * (double)round_up(M + 1, kGdKT) * (double)cols;
        }
        timer.mark(kGdRoot, s);
        CAFE_LAUNCH(c, gain_dense_root_kernel, dim3((unsigned)(cols / 64)), dim3(256), 0, s, ra);
        timer.mark(kGdRoot, s);
        HIP_TRY(c, hipMemcpyAsync(res.data(), base + o_out, sizeof(double) * nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));            // the host tables of this batch go out of use
        std::copy(res.begin(), res.begin() + nb, family_lnl + b0);
    }
    timer.collect(c->gain_dense_ms);
    return CAFE_OK;
}

}  // namespace
}  // namespace cafe

int cafe_score_gain(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent, int64_t n,
                    const int64_t* family, double* family_lnl) {
    const int rc = cafe::guarded(ctx, "cafe_score_gain", [&] { return cafe::score_gain_impl(ctx, params, lambdas, mus, nus, root_absent, n, family, family_lnl); });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

int cafe_debug_gain_dense(cafe_ctx* ctx, double ms[4], double* flops) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    for (int k = 0; ms && k < 4; ++k) ms[k] = ctx->gain_dense_ms[k];
    if (flops) *flops = ctx->gain_dense_flops;
    return CAFE_OK;
}
