// The sum-product engine of the posterior calls -- cafe_marginal_reconstruct (marginal.hip), cafe_sample_histories
// (history.hip), cafe_score_gradient (gradient.hip) and cafe_expected_events (events.hip) -- and the host frame they share (sum_product.h).
// Panels, matrices and the two passes are described in marginal.hip's header comment.
#include <cmath>

#include "sum_product.h"

namespace cafe {

namespace {

// ---------------------------------------------------------------------------------------------------------------- GEMM
// Block tile 64 rows x 128 families, K step 16; wave w owns the 32 families 32w.. over all 64 rows: 4 x 2 accumulator tiles
// of v_mfma_f64_16x16x4_f64 (A fragment: row = lane & 15, k = lane >> 4; B fragment: k = lane >> 4, column = lane & 15;
// D: row = (lane >> 4) + 4 * register, column = lane & 15).  Both tiles are staged in LDS k-major with a 16-double pad, so
// that the four k rows a fragment load touches start 32 banks apart.  The next K step's global loads are in flight while
// the current one is multiplied.  Every load is guarded by the matrix's extent: nothing depends on padding rows.
constexpr int kMT = 64, kNT = 128, kKT = 16;
constexpr int kLdA = kMT + 16, kLdX = kNT + 16;

template <int MODE, bool MUL>
__global__ __launch_bounds__(256) void marginal_gemm_kernel(const GemmParams a) {
    __shared__ __attribute__((aligned(16))) double As[kKT * kLdA];
    __shared__ __attribute__((aligned(16))) double Xs[kKT * kLdX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int r0 = blockIdx.y * kMT;
    const int64_t c0 = (int64_t)blockIdx.x * kNT;
    const int nr = a.nr, nk = a.nk, ldp = a.ldp;
    const int64_t ld = a.ld;
    // split: the K tiles strictly off the diagonal run whole (or not at all), the ones that meet it take the mask
    int kbeg = 0, kend = nk;
    if (MODE == kSplit) {
        if (a.mask == 1) kend = min(nk, r0 + kMT - 1);       // i < j <= r0 + 63, i = k + 1
        else kbeg = r0;                                      // i > j >= r0
    }
    typedef double d4 __attribute__((ext_vector_type(4)));
    d4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
    double ra[4];
    double2 rx[4];
    const int xoff = MODE == kUp ? 0 : 1;
    auto load = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (MODE == kUp) {                               // A[r][k] = Pt[k][r]: 64 consecutive rows per k
                const int r = r0 + lane, k = k0 + wave + 4 * u;
                ra[u] = (r < nr && k < nk) ? a.Pt[(int64_t)k * ldp + r] : 0.0;
            } else {                                         // A[r][k] = Pt[r][k]: 16 consecutive k per row
                const int k = k0 + (tid & 15), r = r0 + (tid >> 4) + 16 * u;
                bool ok = r < nr && k < nk;
                if (MODE == kSplit) ok = ok && (a.mask == 1 ? k + 1 < r : k + 1 > r);
                ra[u] = ok ? a.Pt[(int64_t)r * ldp + k] : 0.0;
            }
            const int k = k0 + wave + 4 * u;
            rx[u] = k < nk ? *reinterpret_cast<const double2*>(a.X + (int64_t)(k + xoff) * ld + c0 + 2 * lane) : make_double2(0.0, 0.0);
        }
    };
    if (kbeg < kend) load(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += kKT) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (MODE == kUp) As[(wave + 4 * u) * kLdA + lane] = ra[u];
            else As[(tid & 15) * kLdA + (tid >> 4) + 16 * u] = ra[u];
            *reinterpret_cast<double2*>(&Xs[(wave + 4 * u) * kLdX + 2 * lane]) = rx[u];
        }
        __syncthreads();
        if (k0 + kKT < kend) load(k0 + kKT);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            double af[4], bf[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = As[(4 * s4 + l4) * kLdA + 16 * i + l15];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Xs[(4 * s4 + l4) * kLdX + 32 * wave + 16 * j + l15];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    // ---- epilogue
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 16 * i + l4 + 4 * q;
                if (r >= nr) continue;
                const int64_t c = c0 + 32 * wave + 16 * j + l15;
                double v = acc[i][j][q];
                if (MODE == kUp) {                           // parent size r + 1
                    const int64_t o = (int64_t)(r + 1) * ld + c;
                    a.out1[o] = v;
                    a.out2[o] = MUL ? a.out2[o] * v : v;
                } else if (MODE == kDown) {
                    const int64_t o = (int64_t)r * ld + c;
                    if (r == 0) v += a.X[c];                 // P[0][j] = delta(j, 0)
                    a.out1[o] = v;
                    const double t = a.pk * (v * a.Bv[o]);
                    a.out2[o] = a.first ? t : a.out2[o] + t;
                } else {
                    const int64_t o = (int64_t)r * ld + c;
                    a.out1[o] = v * a.Bv[o];
                }
            }
    if (MODE == kUp && blockIdx.y == 0 && tid < kNT) {       // F[0] = B_v[0]
        const int64_t c = c0 + tid;
        const double v = a.X[c];
        a.out1[c] = v;
        a.out2[c] = MUL ? a.out2[c] * v : v;
    }
}

// The scorer's leaf factor (leaf_reduce.hip): P[i][x], or with an error model sum_t err[x][t] P[i][x - half + t], taps
// outside [0, M] dropped, in the scorer's tap order.  A missing cell's factor is exactly 1.0 (cafe_kernels.h); the posterior
// calls built on this unit refuse a context that has one (guarded_observed, cafe_call.h), all but the leave-one-out check.
__device__ inline double leaf_factor(const double* __restrict__ P, int ldp, int i, int x, const double* __restrict__ err, int n_dev, int M) {
    if (count_is_missing(x)) return leaf_factor_or_one(x, 0.0);
    const double* row = P + (int64_t)i * ldp;
    if (err == nullptr) return row[x];
    const int half = (n_dev - 1) / 2;
    double fac = 0.0;
    for (int t = 0; t < n_dev; ++t) {
        const int c = x - half + t;
        if (c < 0 || c > M) continue;
        fac += row[c] * err[(int64_t)x * n_dev + t];
    }
    return fac;
}

// dst[i][f] = (src0 ? src0[i][f] : 1) * prod panels[i][f] * prod leaf factors(i, x_f), i = 0..rows-1.  The up pass forms the
// product of a node's leaf children with it, the down pass G_v = O_parent * the siblings' factors.
constexpr int kMaxProd = 6;
struct ProdParams {
    const double* src0;
    double* dst;
    int64_t ld;
    int rows;
    int n_pan, n_leaf;
    const double* pan[kMaxProd];
    const double* P[kMaxProd];          // row-major matrices of the leaf branches
    const int32_t* cnt[kMaxProd];       // observed counts of the batch's columns
    int ldp;
    const double* err;
    int n_dev, M;
};
__global__ __launch_bounds__(256) void marginal_product_kernel(const ProdParams a) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= a.ld) return;
    int x[kMaxProd];
#pragma unroll
    for (int l = 0; l < kMaxProd; ++l) x[l] = l < a.n_leaf ? a.cnt[l][f] : 0;
    const int i0 = blockIdx.y * 16, i1 = min(a.rows, i0 + 16);
    for (int i = i0; i < i1; ++i) {
        const int64_t o = (int64_t)i * a.ld + f;
        double v = a.src0 ? a.src0[o] : 1.0;
#pragma unroll
        for (int p = 0; p < kMaxProd; ++p)
            if (p < a.n_pan) v *= a.pan[p][o];
#pragma unroll
        for (int l = 0; l < kMaxProd; ++l)
            if (l < a.n_leaf) v *= leaf_factor(a.P[l], a.ldp, i, x[l], a.err, a.n_dev, a.M);
        a.dst[o] = v;
    }
}

}  // namespace

template <int MODE>
int launch_gemm(cafe_ctx* c, const GemmParams& g, bool mul, hipStream_t s, GemmTimer& timer, double share) {
    dim3 grid((unsigned)(g.ld / kNT), (unsigned)((g.nr + kMT - 1) / kMT));
    timer.mark(s);
    if constexpr (MODE == kUp) {
        if (mul) CAFE_LAUNCH(c, (marginal_gemm_kernel<kUp, true>), grid, dim3(256), 0, s, g);
    }
    if (MODE != kUp || !mul) CAFE_LAUNCH(c, (marginal_gemm_kernel<MODE, false>), grid, dim3(256), 0, s, g);
    timer.mark(s);
    timer.flops += share * 2.0 * g.nr * g.nk * (double)g.ld;
    return CAFE_OK;
}

template int launch_gemm<kUp>(cafe_ctx*, const GemmParams&, bool, hipStream_t, GemmTimer&, double);
template int launch_gemm<kDown>(cafe_ctx*, const GemmParams&, bool, hipStream_t, GemmTimer&, double);
template int launch_gemm<kSplit>(cafe_ctx*, const GemmParams&, bool, hipStream_t, GemmTimer&, double);

int marginal_product(cafe_ctx* c, const UpPanels& w, const double* src0, double* dst, int nrows, const std::vector<int>& mult, int k, int64_t f0, int64_t ld,
                     hipStream_t s) {
    const unsigned gb = (unsigned)((ld + 255) / 256);
    size_t i = 0;
    bool started = false;
    while (i < mult.size() || !started) {
        ProdParams p{};
        p.src0 = started ? dst : src0;
        p.dst = dst; p.ld = ld; p.rows = nrows; p.ldp = c->pool.ld; p.err = w.err; p.n_dev = w.n_dev; p.M = c->M;
        for (; i < mult.size(); ++i) {
            const int m = mult[i];
            if (c->leaf_taxon[m] >= 0) {
                if (p.n_leaf == kMaxProd) break;
                p.P[p.n_leaf] = leaf_matrix(c, m, k);
                p.cnt[p.n_leaf] = leaf_counts(c, m, f0);
                ++p.n_leaf;
            } else {
                if (p.n_pan == kMaxProd) break;
                p.pan[p.n_pan++] = w.panel(w.F, m);
            }
        }
        CAFE_LAUNCH(c, marginal_product_kernel, dim3(gb, (unsigned)((nrows + 15) / 16)), dim3(256), 0, s, p);
        started = true;
    }
    return CAFE_OK;
}

// children before parents: the node order of the problem
int marginal_up_pass(cafe_ctx* c, const UpPanels& w, int k, int64_t f0, int64_t ld, hipStream_t s, GemmTimer& timer) {
    const int M = c->M, R = c->R, n = c->n_nodes;
    for (int p = 0; p < n; ++p) {
        if (c->leaf_taxon[p] >= 0) continue;
        const int np = p == c->root ? R : M;          // parent sizes 1..np
        std::vector<int> leaves;
        for (int v : c->children[p]) if (c->leaf_taxon[v] >= 0) leaves.push_back(v);
        bool started = false;
        if (!leaves.empty()) {
            const int rc = marginal_product(c, w, nullptr, w.panel(w.B, p), np + 1, leaves, k, f0, ld, s);
            if (rc != CAFE_OK) return rc;
            started = true;
        }
        for (int v : c->children[p]) {
            if (c->leaf_taxon[v] >= 0) continue;
            GemmParams g{};
            g.Pt = interior_matrix(c, v, k);
            g.ldp = c->kpool.ld; g.X = w.panel(w.B, v); g.ld = ld; g.nr = np; g.nk = M + 1;
            g.out1 = w.panel(w.F, v); g.out2 = w.panel(w.B, p);
            if (const int rc = launch_gemm<kUp>(c, g, started, s, timer)) return rc;
            started = true;
        }
    }
    return CAFE_OK;
}

std::vector<Branch> branches_down(const cafe_ctx* c) {
    std::vector<Branch> out;
    for (int p = c->n_nodes - 1; p >= 0; --p)
        for (int v : c->children[p]) {                       // (a leaf has none)
            out.push_back({p, v, p == c->root ? c->R : c->M, {}});
            for (int w : c->children[p]) if (w != v) out.back().sib.push_back(w);
        }
    return out;
}

int down_branch(cafe_ctx* c, const UpPanels& w, double* O, double* G, const Branch& b, int k, double pk, int64_t f0, int64_t ld, hipStream_t s, GemmParams* g) {
    *g = GemmParams{};
    if (c->leaf_taxon[b.v] < 0) {
        g->Pt = interior_matrix(c, b.v, k);
        g->ldp = c->kpool.ld; g->X = G; g->ld = ld; g->nr = c->M + 1; g->nk = b.np;
        g->out1 = w.panel(O, b.v); g->Bv = w.panel(w.B, b.v); g->pk = pk;
    }
    return marginal_product(c, w, w.panel(O, b.p), G, b.np + 1, b.sib, k, f0, ld, s);
}

int open_posterior_call(cafe_ctx* c, const cafe_params* pr, PosteriorCall* pc) {
    pc->gamma = pr->model == CAFE_MODEL_GAMMA;
    pc->K = pc->gamma ? pr->n_categories : 1;
    if (const int rc = begin_matrix_call(c, pr->lambdas, pc->gamma ? pr->multipliers : nullptr, pc->K, &pc->s)) return rc;
    pc->has_err = pr->error_model != nullptr;
    pc->n_dev = pc->up.n_dev = pc->has_err ? c->n_dev : 1;
    pc->up.bidx.assign(c->n_nodes, -1);
    for (int v = 0; v < c->n_nodes; ++v) if (c->leaf_taxon[v] < 0) pc->up.bidx[v] = pc->nI++;
    return CAFE_OK;
}

hipError_t alloc_constants(const cafe_ctx* c, PriorLogs logs, PosteriorCall* pc) {
    const size_t o_probs = (logs == kWithPriorLogs ? 2 : 1) * (size_t)c->R, n_err = pc->has_err ? (size_t)(c->M + 1) * pc->n_dev : 0;
    pc->n_consts = o_probs + pc->K + n_err;
    const hipError_t e = hipMalloc(&pc->consts.p, sizeof(double) * pc->n_consts);
    pc->prior = static_cast<const double*>(pc->consts.p);
    pc->logprior = logs == kWithPriorLogs ? pc->prior + c->R : nullptr;
    pc->probs = pc->prior + o_probs;
    pc->up.err = n_err ? pc->probs + pc->K : nullptr;
    return e;
}

int upload_constants(cafe_ctx* c, const cafe_params* pr, PosteriorCall* pc) {
    const size_t R = c->R, K = pc->K, o_probs = pc->probs - pc->prior;
    std::vector<double> h(pc->n_consts, 1.0);                // 1.0: the base model's one weight
    for (size_t j = 0; j < R; ++j) h[j] = (double)pr->prior[j];      // compute() returns a float
    if (pc->logprior) for (size_t j = 0; j < R; ++j) h[R + j] = std::log(h[j]);
    if (pc->gamma) std::copy(pr->cat_probs, pr->cat_probs + K, h.begin() + o_probs);
    if (pc->has_err) std::copy(pr->error_model, pr->error_model + (h.size() - o_probs - K), h.begin() + o_probs + K);
    HIP_TRY(c, hipMemcpyAsync(pc->consts.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, pc->s));
    HIP_TRY(c, hipStreamSynchronize(pc->s));
    return CAFE_OK;
}

}  // namespace cafe
