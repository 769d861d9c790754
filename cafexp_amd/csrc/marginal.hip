// Marginal ancestral reconstruction: posterior size distributions of every node, credible intervals and the posterior
// probability that a branch expanded or contracted.
//
// The model is the scorer's (inference_prune / compute_node_probability, src/core.cpp:133, src/probability.cpp:173-242), not
// the joint reconstructor's variant with L[0] = 0.  With i = size of a node's parent, j = size of the node v, P_v its matrix:
//   up    F_v[i] = sum_j P_v[i][j] B_v[j]          B_p[i] = prod_{children} F_c[i]           leaf: the scorer's gather, taps included
//   root  O_root[s] = prior[s-1], s = 1..R         Z = sum_s O_root[s] B_root[s]
//   down  G_v[i] = O_p[i] prod_{siblings} F_w[i]   O_v[j] = sum_i P_v[i][j] G_v[i]            (products of stored factors: no division)
//   post_v[j] ~ O_v[j] B_v[j];  joint of a branch = G_v[i] P_v[i][j] B_v[j] / Z
// Panels are [size][family], families fastest.  The interior matrices are the k-major ones K1 builds (Pt[j][i-1] = P[i][j],
// row i = 0 of P is e_0 and is not stored), so ONE fp64 MFMA GEMM serves both passes: the up pass reads A[i][j] = Pt[j][i-1]
// (A transposed in memory), the down pass reads the rows of Pt as they lie.  Row 0 of P is added by the epilogue, as K5 does.
// Gamma model: every category runs the same launches; the un-normalised posteriors are accumulated with weight cat_probs[k]
// in one panel per interior node and summarised once (the base model is K = 1).
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "cafe_call.h"
#include "marginal_up.h"

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

// ------------------------------------------------------------------------------------------------------- small kernels
// The scorer's leaf factor (leaf_reduce.hip): P[i][x], or with an error model sum_t err[x][t] P[i][x - half + t], taps
// outside [0, M] dropped, in the scorer's tap order.
__device__ inline double leaf_factor(const double* __restrict__ P, int ldp, int i, int x, const double* __restrict__ err, int n_dev, int M) {
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

// root weighting: O_root[s] = prior[s-1], acc_root[s] (+)= p_k prior[s-1] B_root[s], s = 1..R; row 0 carries no mass
__global__ __launch_bounds__(256) void marginal_root_kernel(const double* __restrict__ B, const double* __restrict__ prior, int R, int64_t ld,
                                                            double* __restrict__ O, double* __restrict__ acc, double pk, int first) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const int s0 = blockIdx.y * 16, s1 = min(R + 1, s0 + 16);
    for (int s = s0; s < s1; ++s) {
        const int64_t o = (int64_t)s * ld + f;
        const double w = s >= 1 ? prior[s - 1] : 0.0;
        O[o] = w;
        const double t = pk * (w * B[o]);
        acc[o] = first ? t : acc[o] + t;
    }
}

// out[f] (+)= p_k sum_j D[j][f]: the masked down GEMM dotted with B_v (its epilogue already multiplied)
__global__ __launch_bounds__(256) void marginal_colsum_kernel(const double* __restrict__ D, int rows, int64_t ld, double* __restrict__ out, double pk, int first) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double s = 0.0;
    for (int j = 0; j < rows; ++j) s += D[(int64_t)j * ld + f];
    out[f] = first ? pk * s : out[f] + pk * s;
}

// A leaf branch: for every tap c of the observed count x (c = x without an error model), sum_i G[i] P[i][c] split at i < c,
// i = c, i > c.  acc[t] (+)= p_k e[t] (whole sum): the posterior over the taps; acc[n_tap] / acc[n_tap + 1]: the mass with
// the leaf above / below its parent.
__global__ __launch_bounds__(256) void marginal_leaf_kernel(const double* __restrict__ G, int rows, int64_t ld, const double* __restrict__ P, int ldp,
                                                            const int32_t* __restrict__ cnt, const double* __restrict__ err, int n_dev, int M,
                                                            double* __restrict__ acc, double pk, int first) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const int x = cnt[f];
    const int n_tap = err ? n_dev : 1, half = err ? (n_dev - 1) / 2 : 0;
    double up = 0.0, down = 0.0;
    for (int t = 0; t < n_tap; ++t) {
        const int c = x - half + t;
        double lt = 0.0, eq = 0.0, gt = 0.0, w = 0.0;
        if (c >= 0 && c <= M) {
            w = err ? err[(int64_t)x * n_dev + t] : 1.0;
            for (int i = 0; i < rows; ++i) {
                const double term = G[(int64_t)i * ld + f] * P[(int64_t)i * ldp + c];
                if (i < c) lt += term;
                else if (i > c) gt += term;
                else eq = term;
            }
        }
        const double tot = pk * (w * (lt + eq + gt));
        double* o = acc + (int64_t)t * ld + f;
        *o = first ? tot : *o + tot;
        up += w * lt;
        down += w * gt;
    }
    double* o = acc + (int64_t)n_tap * ld + f;
    o[0] = first ? pk * up : o[0] + pk * up;
    o[ld] = first ? pk * down : o[ld] + pk * down;
}

struct SummaryOut {
    double* mean;
    int32_t *mode, *lo, *hi;
    double *p_inc, *p_dec;
};

// One walk over a node's accumulated posterior: mean, first arg max and the two CDF crossings.  The root's launch also
// produces Z = sum_s acc_root[s] first; every other node is normalised by that Z.
__global__ __launch_bounds__(256) void marginal_summary_kernel(const double* __restrict__ acc, int jmax, int64_t ld, double* __restrict__ Z, int make_z,
                                                               double level, const double* __restrict__ br_inc, const double* __restrict__ br_dec,
                                                               SummaryOut out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double z;
    if (make_z) {
        z = 0.0;
        for (int j = 0; j <= jmax; ++j) z += acc[(int64_t)j * ld + f];
        Z[f] = z;
    } else {
        z = Z[f];
    }
    const double nan = __builtin_nan("");
    if (!(z > 0.0) || z > 1.7976931348623157e308) {          // Z = 0 or not finite: a failed family
        out.mean[f] = nan; out.mode[f] = -1; out.lo[f] = -1; out.hi[f] = -1; out.p_inc[f] = nan; out.p_dec[f] = nan;
        return;
    }
    const double tlo = 0.5 * (1.0 - level) * z, thi = (1.0 - 0.5 * (1.0 - level)) * z;
    double cum = 0.0, mean = 0.0, best = -1.0;
    int arg = 0, lo = -1, hi = -1;
    for (int j = 0; j <= jmax; ++j) {
        const double p = acc[(int64_t)j * ld + f];
        if (p > best) { best = p; arg = j; }
        cum += p;
        mean += (double)j * p;
        if (lo < 0 && cum >= tlo) lo = j;
        if (hi < 0 && cum >= thi) hi = j;
    }
    out.mean[f] = mean / z;
    out.mode[f] = arg;
    out.lo[f] = lo < 0 ? jmax : lo;
    out.hi[f] = hi < 0 ? jmax : hi;
    out.p_inc[f] = br_inc ? br_inc[f] / z : nan;
    out.p_dec[f] = br_dec ? br_dec[f] / z : nan;
}

// A leaf's row: the observed count, or with an error model the posterior over its taps (marginal_leaf_kernel's sums)
__global__ __launch_bounds__(256) void marginal_leaf_summary_kernel(const double* __restrict__ acc, const int32_t* __restrict__ cnt, int n_dev, int has_err,
                                                                    int M, int64_t ld, const double* __restrict__ Z, double level, SummaryOut out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const double z = Z[f], nan = __builtin_nan("");
    if (!(z > 0.0) || z > 1.7976931348623157e308) {
        out.mean[f] = nan; out.mode[f] = -1; out.lo[f] = -1; out.hi[f] = -1; out.p_inc[f] = nan; out.p_dec[f] = nan;
        return;
    }
    const int x = cnt[f];
    const int n_tap = has_err ? n_dev : 1, half = has_err ? (n_dev - 1) / 2 : 0;
    out.p_inc[f] = acc[(int64_t)n_tap * ld + f] / z;
    out.p_dec[f] = acc[(int64_t)(n_tap + 1) * ld + f] / z;
    if (!has_err) {
        out.mean[f] = (double)x; out.mode[f] = x; out.lo[f] = x; out.hi[f] = x;
        return;
    }
    const double tlo = 0.5 * (1.0 - level) * z, thi = (1.0 - 0.5 * (1.0 - level)) * z;
    double cum = 0.0, mean = 0.0, best = -1.0;
    int arg = 0, lo = -1, hi = -1, last = 0;
    for (int t = 0; t < n_tap; ++t) {
        const int c = x - half + t;
        if (c < 0 || c > M) continue;
        const double p = acc[(int64_t)t * ld + f];
        if (p > best) { best = p; arg = c; }
        cum += p;
        mean += (double)c * p;
        if (lo < 0 && cum >= tlo) lo = c;
        if (hi < 0 && cum >= thi) hi = c;
        last = c;
    }
    out.mean[f] = mean / z;
    out.mode[f] = arg;
    out.lo[f] = lo < 0 ? last : lo;
    out.hi[f] = hi < 0 ? last : hi;
}

}  // namespace

// One GEMM launch between the timer's marks; share: the part of its K tiles that runs (declared in marginal_up.h, which
// cafe_score_gradient shares it through)
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

// dst = (src0) * the factors of `mult` (interior: stored F panels, leaves: gathered), rows 0..nrows-1
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

// The up pass of category k over the columns f0 .. f0 + ld: children before parents (node order of the problem)
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

int marginal_impl(cafe_ctx* c, const cafe_params* pr, double level, const cafe_marginal_out* out) {
    if (c->comm) { set_err(c, "cafe_marginal_reconstruct: not valid on a context with a communicator attached"); return CAFE_ERR_STATE; }
    if (!pr || !pr->lambdas || !pr->prior || !out) { set_err(c, "cafe_marginal_reconstruct: lambdas, prior and out are required"); return CAFE_ERR_ARGUMENT; }
    if (!(level > 0.0 && level < 1.0)) { set_err(c, "cafe_marginal_reconstruct: level must lie in (0, 1)"); return CAFE_ERR_ARGUMENT; }
    const bool gamma = pr->model == CAFE_MODEL_GAMMA;
    const int K = gamma ? pr->n_categories : 1;
    if (gamma && (K < 1 || K > c->Kmax || !pr->multipliers || !pr->cat_probs)) {
        set_err(c, "cafe_marginal_reconstruct: gamma model needs 1..%d categories with multipliers and cat_probs", c->Kmax);
        return CAFE_ERR_ARGUMENT;
    }
    if (!rates_valid(c, pr->lambdas)) { set_err(c, "cafe_marginal_reconstruct: invalid lambda or death rate"); return CAFE_ERR_ARGUMENT; }
    if (pr->error_model && c->n_dev < 1) { set_err(c, "cafe_marginal_reconstruct: the context was created without an error model"); return CAFE_ERR_ARGUMENT; }
    hipStream_t s = nullptr;
    if (const int rc = begin_matrix_call(c, pr->lambdas, gamma ? pr->multipliers : nullptr, K, &s)) return rc;

    const int M = c->M, R = c->R, n = c->n_nodes, rows = c->N;      // a panel holds sizes 0..max(M, R)
    const bool has_err = pr->error_model != nullptr;
    const int n_dev = has_err ? c->n_dev : 1, n_tap = n_dev;
    UpPanels up;
    std::vector<int>& bidx = up.bidx;
    std::vector<int> lidx(n, -1);
    bidx.assign(n, -1);
    int nI = 0, nL = 0;
    for (int v = 0; v < n; ++v) { if (c->leaf_taxon[v] < 0) bidx[v] = nI++; else lidx[v] = nL++; }

    // workspace per column: B, F, O and the accumulation panel of every interior node, G and D, the leaf sums, the branch
    // sums, Z and the summaries
    const size_t dbl_per_col = (size_t)4 * nI * rows + 2 * (size_t)rows + (size_t)nL * (n_tap + 2) + 2 * (size_t)nI + 1 + 3 * (size_t)n;
    const size_t per_col = dbl_per_col * sizeof(double) + (size_t)3 * n * sizeof(int32_t);
    int64_t cols = 0;
    if (const int rc = column_chunk(c, per_col, "cafe_marginal_reconstruct: not enough device memory for the panels of " + std::to_string(nI) + " interior nodes", &cols))
        return rc;
    DevBuf wd, wi, dprior, derr;
    if (hipMalloc(&wd.p, dbl_per_col * cols * sizeof(double)) != hipSuccess || hipMalloc(&wi.p, (size_t)3 * n * cols * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&dprior.p, sizeof(double) * R) != hipSuccess ||
        (has_err && hipMalloc(&derr.p, sizeof(double) * (size_t)(M + 1) * n_dev) != hipSuccess)) {
        (void)hipGetLastError();
        set_err(c, "cafe_marginal_reconstruct: cannot allocate the workspace (%lld columns)", (long long)cols);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemsetAsync(wd.p, 0, dbl_per_col * cols * sizeof(double), s));
    const int64_t pstride = (int64_t)rows * cols;
    double* base = static_cast<double*>(wd.p);
    double* d_B = base;
    double* d_F = d_B + (int64_t)nI * pstride;
    double* d_O = d_F + (int64_t)nI * pstride;
    double* d_A = d_O + (int64_t)nI * pstride;
    double* d_G = d_A + (int64_t)nI * pstride;
    double* d_D = d_G + pstride;
    double* d_leaf = d_D + pstride;                          // [leaf][n_tap + 2][cols]
    double* d_br = d_leaf + (int64_t)nL * (n_tap + 2) * cols;      // [interior node][2][cols]
    double* d_Z = d_br + (int64_t)2 * nI * cols;
    double* d_mean = d_Z + cols;                             // [node][cols]
    double* d_pinc = d_mean + (int64_t)n * cols;
    double* d_pdec = d_pinc + (int64_t)n * cols;
    int32_t* d_mode = static_cast<int32_t*>(wi.p);
    int32_t* d_lo = d_mode + (int64_t)n * cols;
    int32_t* d_hi = d_lo + (int64_t)n * cols;
    {
        std::vector<double> hp(R);
        for (int j = 0; j < R; ++j) hp[j] = (double)pr->prior[j];          // compute() returns a float
        HIP_TRY(c, hipMemcpyAsync(dprior.p, hp.data(), sizeof(double) * R, hipMemcpyHostToDevice, s));
        if (has_err) HIP_TRY(c, hipMemcpyAsync(derr.p, pr->error_model, sizeof(double) * (size_t)(M + 1) * n_dev, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    const double* d_prior = static_cast<const double*>(dprior.p);
    const double* d_err = has_err ? static_cast<const double*>(derr.p) : nullptr;
    up.B = d_B; up.F = d_F; up.pstride = pstride; up.err = d_err; up.n_dev = n_dev;

    GemmTimer timer;
    timer.on = c->profile != 0;
    std::vector<double> h_mean((size_t)n * cols), h_pinc((size_t)n * cols), h_pdec((size_t)n * cols), h_Z(cols);
    std::vector<int32_t> h_mode((size_t)n * cols), h_lo((size_t)n * cols), h_hi((size_t)n * cols);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int64_t f0 = 0; f0 < c->Fp; f0 += cols) {
        const int64_t ld = std::min<int64_t>(cols, c->Fp - f0);
        const unsigned gb = (unsigned)((ld + 255) / 256);
        auto panel = [&](double* arena, int v) { return arena + (int64_t)bidx[v] * pstride; };
        auto product = [&](const double* src0, double* dst, int nrows, const std::vector<int>& mult, int k) {
            return marginal_product(c, up, src0, dst, nrows, mult, k, f0, ld, s);
        };
        for (int k = 0; k < K; ++k) {
            const double pk = gamma ? pr->cat_probs[k] : 1.0;
            const int first = k == 0;
            // ---- up: children before parents (marginal_up_pass, shared with cafe_sample_histories)
            if (const int rc = marginal_up_pass(c, up, k, f0, ld, s, timer)) return rc;
            // ---- root, then parents before children
            CAFE_LAUNCH(c, marginal_root_kernel, dim3(gb, (unsigned)((R + 1 + 15) / 16)), dim3(256), 0, s, panel(d_B, c->root), d_prior, R, ld, panel(d_O, c->root),
                        panel(d_A, c->root), pk, first);
            for (int p = n - 1; p >= 0; --p) {
                if (c->leaf_taxon[p] >= 0) continue;
                const int np = p == c->root ? R : M;
                for (int v : c->children[p]) {
                    std::vector<int> sib;
                    for (int w : c->children[p]) if (w != v) sib.push_back(w);
                    { const int rc = product(panel(d_O, p), d_G, np + 1, sib, k); if (rc != CAFE_OK) return rc; }
                    if (c->leaf_taxon[v] >= 0) {
                        CAFE_LAUNCH(c, marginal_leaf_kernel, dim3(gb), dim3(256), 0, s, d_G, np + 1, ld, leaf_matrix(c, v, k), c->pool.ld, leaf_counts(c, v, f0), d_err,
                                    n_dev, M, d_leaf + (int64_t)lidx[v] * (n_tap + 2) * cols, pk, first);
                        continue;
                    }
                    GemmParams g{};
                    g.Pt = interior_matrix(c, v, k);
                    g.ldp = c->kpool.ld; g.X = d_G; g.ld = ld; g.nr = M + 1; g.nk = np;
                    g.out1 = panel(d_O, v); g.out2 = panel(d_A, v); g.Bv = panel(d_B, v); g.pk = pk; g.first = first;
                    if (const int rc = launch_gemm<kDown>(c, g, false, s, timer)) return rc;
                    for (int m = 1; m <= 2; ++m) {           // the branch split: i < j, then i > j
                        g.mask = m; g.out1 = d_D; g.out2 = nullptr;
                        if (const int rc = launch_gemm<kSplit>(c, g, false, s, timer, 0.5)) return rc;      // about half of the K tiles run
                        CAFE_LAUNCH(c, marginal_colsum_kernel, dim3(gb), dim3(256), 0, s, d_D, M + 1, ld, d_br + ((int64_t)2 * bidx[v] + (m - 1)) * cols, pk, first);
                    }
                }
            }
        }
        // ---- summaries: the root first (it makes Z)
        for (int pass = 0; pass < 2; ++pass)
            for (int v = 0; v < n; ++v) {
                if ((v == c->root) != (pass == 0)) continue;
                SummaryOut so{d_mean + (int64_t)v * cols, d_mode + (int64_t)v * cols, d_lo + (int64_t)v * cols, d_hi + (int64_t)v * cols,
                              d_pinc + (int64_t)v * cols, d_pdec + (int64_t)v * cols};
                if (c->leaf_taxon[v] >= 0) {
                    CAFE_LAUNCH(c, marginal_leaf_summary_kernel, dim3(gb), dim3(256), 0, s, d_leaf + (int64_t)lidx[v] * (n_tap + 2) * cols, leaf_counts(c, v, f0), n_dev,
                                has_err ? 1 : 0, M, ld, d_Z, level, so);
                } else {
                    const bool is_root = v == c->root;
                    const double* bi = is_root ? nullptr : d_br + (int64_t)2 * bidx[v] * cols;
                    CAFE_LAUNCH(c, marginal_summary_kernel, dim3(gb), dim3(256), 0, s, panel(d_A, v), is_root ? R : M, ld, d_Z, is_root ? 1 : 0, level, bi,
                                bi ? bi + cols : nullptr, so);
                }
            }
        HIP_TRY(c, hipMemcpyAsync(h_mean.data(), d_mean, sizeof(double) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_pinc.data(), d_pinc, sizeof(double) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_pdec.data(), d_pdec, sizeof(double) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_mode.data(), d_mode, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_lo.data(), d_lo, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_hi.data(), d_hi, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_Z.data(), d_Z, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for_each_family_of_chunk(c, f0, ld, [&](int64_t f, int64_t col) {
            const double z = h_Z[col];
            const bool bad = !(z > 0.0) || !std::isfinite(z);
            if (out->log_evidence) out->log_evidence[f] = bad ? nan : std::log(z);
            if (out->failed) out->failed[f] = bad ? 1 : 0;
            for (int v = 0; v < n; ++v) {
                const size_t src = (size_t)v * cols + col, dst = (size_t)f * n + v;
                if (out->mean) out->mean[dst] = h_mean[src];
                if (out->mode) out->mode[dst] = h_mode[src];
                if (out->lo) out->lo[dst] = h_lo[src];
                if (out->hi) out->hi[dst] = h_hi[src];
                if (out->p_increase) out->p_increase[dst] = h_pinc[src];
                if (out->p_decrease) out->p_decrease[dst] = h_pdec[src];
            }
        });
    }
    c->upload_pending = false;
    // the matrices of this call stay readable (cafe_get_matrix); per-family scorer results are not meaningful
    c->have_results = true;
    c->rootmax_last = true;
    c->last_rejected = false;
    c->marginal_gemm_ms = timer.on ? timer.total_ms() : 0.0;
    c->marginal_gemm_flops = timer.flops;
    return CAFE_OK;
}

}  // namespace cafe

extern "C" {

int cafe_marginal_reconstruct(cafe_ctx* ctx, const cafe_params* params, double level, const cafe_marginal_out* out) {
    return cafe::guarded(ctx, "cafe_marginal_reconstruct", [&] { return cafe::marginal_impl(ctx, params, level, out); });
}

int cafe_debug_marginal_gemm(cafe_ctx* ctx, double* ms, double* flops) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (ms) *ms = ctx->marginal_gemm_ms;
    if (flops) *flops = ctx->marginal_gemm_flops;
    return CAFE_OK;
}

}
