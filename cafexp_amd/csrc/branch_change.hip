// Posterior of each branch's size change: for every family and non-root node v the distribution of
// Delta = size(v) - size(parent(v)) given the leaf counts, in a band of +-D with both tails.
//
// The model, panels and passes are cafe_marginal_reconstruct's (marginal.hip's header comment): the call's lambdas, categories,
// prior and error model, the context's death rates when set, the root weight of the sum rule.  For a non-root node v with
// parent p, category k and column f, i the parent's size and j the node's:
//     J_k[i][j] = G_v^k[i] P_v^k[i][j] B_v^k[j]           i = 0..np (np = R under the root, else M), j = 0..M, P[0][j] = delta(j, 0)
//     w[d]      = sum_k p_k sum_i J_k[i][i + d]           d = -D..D, terms with i + d outside 0..M absent
//     below     = sum_k p_k sum_{j - i < -D} J_k[i][j]    above = sum_k p_k sum_{j - i > D} J_k[i][j]
// all divided by Z = sum_k p_k Z_k at the end.  A leaf branch without an error model has j fixed at the observed x:
// w[d] = G[x - d] P[x - d][x]; with one, Delta is (true size c_t) - i with weights err[x][t] G[i] P[i][c_t], the taps in the
// scorer's order, taps outside 0..M dropped.  Every w[d] is summed in the order of i, then over t, then over k, each product
// formed the same way whatever block of d holds it: a w[d] has the same bits whatever D, workspace limit or column batch the call
// ran with.  The tails are sums of their own, never complements.  mean = E[X_v] - E[X_p] comes from the two nodes' posteriors
// (the accumulation panels of marginal.hip), exact over the whole range, not from the band.
//
// Kernels: the band of an interior branch runs along the diagonals of the joint the sum-product unit forms by rows (lanes are
// columns, a block of kBandD accumulators per lane, the i loop outermost, the matrix entries -- the same for every lane --
// staged in LDS and read as broadcasts); its tails are the masked down GEMM of sum_product.hip with the mask moved D off the
// diagonal; one thread per column walks a leaf branch; a last kernel normalises and summarises.
#include <cmath>
#include <string>
#include <vector>

#include "sum_product.h"

namespace cafe {

namespace {

// root weighting: O_root[s] = prior[s-1], acc_root[s] (+)= p_k prior[s-1] B_root[s], s = 1..R; row 0 carries no mass
__global__ __launch_bounds__(256) void change_root_kernel(const double* __restrict__ B, const double* __restrict__ prior, int R, int64_t ld,
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

// ---------------------------------------------------------------------------------------------------------------- band
// One wave per block, one lane per column, kBandD consecutive values of d per block (blockIdx.y), the parent's size i
// outermost in blocks of the 16 sizes one extent entry covers.  The matrix entries P[i][i + d] = Pt[(i + d) ldp + i - 1] of a
// block -- 16 x kBandD, the same for every lane -- are staged in LDS (eight lanes read the eight consecutive i that one row
// j of Pt gives the band; entries outside the matrix or beyond D are staged as 0) and read back as broadcasts.  The kBandD
// rows of B_v a lane needs move down by one per i: they are kept in a register window, one new row per i, so a step costs
// one load of G and one of B for kBandD multiply-adds.  Rows outside 0..M are clamped: their matrix entry is the staged 0.
// A block of i whose band rows lie outside the matrix, or outside the extent of its 16 columns of Pt (entries that are
// exactly 0), is left out: that changes no bit.  ld is a multiple of 128, so no lane is beyond the batch.
constexpr int kBandD = 8;
constexpr int kBandI = 16;
constexpr int kBandThreads = 64;

struct BandParams {
    const double* Pt;       // k-major matrix of the branch above v: Pt[j ldp + i - 1] = P[i][j]
    int ldp;
    const double* G;        // rows = sizes 0..np of v's parent
    const double* B;        // rows = sizes 0..M of v
    int64_t ld;
    int np, M, D;
    const int32_t* ext;     // interior_extents of the matrix, or nullptr
    double* acc;            // [2D + 1][stride] of the node
    int64_t stride;
    double pk;
    int first;
};

__global__ __launch_bounds__(kBandThreads) void change_band_kernel(const BandParams a) {
    __shared__ __attribute__((aligned(16))) double tile[kBandI * kBandD];      // [i - i0][d - d0]
    const int lane = threadIdx.x;
    const int64_t f = (int64_t)blockIdx.x * kBandThreads + lane;
    const int d0 = -a.D + (int)blockIdx.y * kBandD;
    const int np = a.np, M = a.M, ldp = a.ldp;
    const int64_t ld = a.ld;
    const double* __restrict__ G = a.G + f;
    const double* __restrict__ B = a.B + f;
    double s[kBandD];
    const double row0 = G[0] * B[0];                        // i = 0: P[0][j] = delta(j, 0), so d = 0 alone
#pragma unroll
    for (int e = 0; e < kBandD; ++e) s[e] = d0 + e == 0 ? row0 : 0.0;
    for (int ib = 0; kBandI * ib < np; ++ib) {
        const int i0 = kBandI * ib + 1, i1 = min(np, i0 + kBandI - 1);
        const int jlo = max(i0 + d0, 0), jhi = min(i1 + d0 + kBandD - 1, M);
        if (jlo > jhi) continue;
        if (a.ext) {
            const int e_first = a.ext[2 * ib], e_last = a.ext[2 * ib + 1];
            if (e_first > e_last || jlo > e_last || jhi < e_first) continue;
        }
        __syncthreads();
        {                                                   // stage: row j = i0 + d0 + jr holds the band's i = j - d0 - 7 .. j - d0
            const int q = lane & 7;
#pragma unroll
            for (int pass = 0; pass < 3; ++pass) {
                const int jr = 8 * pass + (lane >> 3), u = jr - (kBandD - 1) + q, e = kBandD - 1 - q;
                const int j = i0 + d0 + jr, i = i0 + u;
                if (u < 0 || u >= kBandI) continue;         // (jr = 23 has no entry either)
                const bool ok = j >= 0 && j <= M && i <= i1 && d0 + e <= a.D;
                tile[u * kBandD + e] = ok ? a.Pt[(int64_t)j * ldp + i - 1] : 0.0;
            }
        }
        __syncthreads();
        double win[kBandD];                                 // win[(u + e) % kBandD] = B[i + d0 + e] at step u of a group
#pragma unroll
        for (int e = 0; e < kBandD - 1; ++e) win[e] = B[(int64_t)min(max(i0 + d0 + e, 0), M) * ld];
        for (int g8 = 0; g8 < kBandI; g8 += kBandD) {
#pragma unroll
            for (int u = 0; u < kBandD; ++u) {
                const int i = i0 + g8 + u;
                win[(u + kBandD - 1) % kBandD] = B[(int64_t)min(max(i + d0 + kBandD - 1, 0), M) * ld];
                const double g = G[(int64_t)min(i, i1) * ld];
#pragma unroll
                for (int e = 0; e < kBandD; ++e) s[e] = __builtin_fma(g * tile[(g8 + u) * kBandD + e], win[(u + e) % kBandD], s[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kBandD; ++e) {
        const int d = d0 + e;
        if (d > a.D) continue;
        double* o = a.acc + (int64_t)(d + a.D) * a.stride + f;
        const double t = a.pk * s[e];
        *o = a.first ? t : *o + t;
    }
}

// ---------------------------------------------------------------------------------------------------------------- tails
// out[j][f] = B_v[j][f] sum_i P[i][j] G[i][f] over i + D < j (mask 1: the node above the band) or i > j + D (mask 2: below it):
// sum_product.hip's down form and tile geometry (block tile 64 rows x 128 families, K step 16, 4 x 2 accumulator tiles of
// v_mfma_f64_16x16x4_f64 per wave, both tiles staged in LDS k-major with a 16-double pad, the next K step's loads in flight),
// with the mask D off the diagonal.  K tiles wholly outside the mask do not run.  Row i = 0 of P never lies in a tail.
constexpr int kMT = 64, kNT = 128, kKT = 16;
constexpr int kLdA = kMT + 16, kLdX = kNT + 16;

struct TailGemm {
    const double* Pt;
    int ldp;
    const double* G;        // rows = parent sizes 0..nk
    const double* Bv;
    int64_t ld;
    int nr, nk;             // sizes 0..nr-1 of v; parent sizes 1..nk
    int mask, D;
    double* out;            // [nr][ld]
};

__global__ __launch_bounds__(256) void change_tail_gemm_kernel(const TailGemm a) {
    __shared__ __attribute__((aligned(16))) double As[kKT * kLdA];
    __shared__ __attribute__((aligned(16))) double Xs[kKT * kLdX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int r0 = blockIdx.y * kMT;
    const int64_t c0 = (int64_t)blockIdx.x * kNT;
    const int nr = a.nr, nk = a.nk, ldp = a.ldp, D = a.D;
    const int64_t ld = a.ld;
    int kbeg = 0, kend = nk;                                 // k = i - 1
    if (a.mask == 1) kend = max(0, min(nk, r0 + kMT - 1 - D));      // i + D < j <= r0 + 63
    else kbeg = r0 + D;                                      // i > j + D >= r0 + D
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
            {                                                // A[r][k] = Pt[r][k]: 16 consecutive k per row
                const int k = k0 + (tid & 15), r = r0 + (tid >> 4) + 16 * u;
                const bool ok = r < nr && k < nk && (a.mask == 1 ? k + 1 + D < r : k + 1 > r + D);
                ra[u] = ok ? a.Pt[(int64_t)r * ldp + k] : 0.0;
            }
            const int k = k0 + wave + 4 * u;
            rx[u] = k < nk ? *reinterpret_cast<const double2*>(a.G + (int64_t)(k + 1) * ld + c0 + 2 * lane) : make_double2(0.0, 0.0);
        }
    };
    if (kbeg < kend) load(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += kKT) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            As[(tid & 15) * kLdA + (tid >> 4) + 16 * u] = ra[u];
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
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 16 * i + l4 + 4 * q;
                if (r >= nr) continue;
                const int64_t o = (int64_t)r * ld + c0 + 32 * wave + 16 * j + l15;
                a.out[o] = acc[i][j][q] * a.Bv[o];
            }
}

// out[f] (+)= p_k sum_j T[j][f]: a tail panel summed over the node's sizes
__global__ __launch_bounds__(256) void change_colsum_kernel(const double* __restrict__ T, int rows, int64_t ld, double* __restrict__ out, double pk, int first) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double s = 0.0;
    for (int j = 0; j < rows; ++j) s += T[(int64_t)j * ld + f];
    out[f] = first ? pk * s : out[f] + pk * s;
}

// ---------------------------------------------------------------------------------------------------------------- leaf
// A leaf branch: for every tap c of the observed count x (c = x without an error model) the terms err[x][t] G[i] P[i][c] over
// i = 0..np (row 0 of a leaf's row-major matrix is stored).  The band entry of d takes the one term i = c - d of every tap, in tap
// order; one walk over i per tap adds the terms beyond the band into the two tails and the whole sum, times c, into the
// node's mean.  acc: [2D + 3][stride], the band, then below, then above; nm: the numerator of E[X_v].
__global__ __launch_bounds__(256) void change_leaf_kernel(const double* __restrict__ G, int rows, int64_t ld, const double* __restrict__ P, int ldp,
                                                          const int32_t* __restrict__ cnt, const double* __restrict__ err, int n_dev, int M, int D,
                                                          double* __restrict__ acc, int64_t stride, double* __restrict__ nm, double pk, int first) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const int x = cnt[f];
    const int n_tap = err ? n_dev : 1, half = err ? (n_dev - 1) / 2 : 0;
    for (int d = -D; d <= D; ++d) {
        double s = 0.0;
        for (int t = 0; t < n_tap; ++t) {
            const int c = x - half + t, i = c - d;
            if (c < 0 || c > M || i < 0 || i >= rows) continue;
            const double w = err ? err[(int64_t)x * n_dev + t] : 1.0;
            s += w * (G[(int64_t)i * ld + f] * P[(int64_t)i * ldp + c]);
        }
        double* o = acc + (int64_t)(d + D) * stride + f;
        *o = first ? pk * s : *o + pk * s;
    }
    double below = 0.0, above = 0.0, m1 = 0.0;
    for (int t = 0; t < n_tap; ++t) {
        const int c = x - half + t;
        if (c < 0 || c > M) continue;
        const double w = err ? err[(int64_t)x * n_dev + t] : 1.0;
        double lo = 0.0, hi = 0.0, tot = 0.0;
        for (int i = 0; i < rows; ++i) {
            const double term = G[(int64_t)i * ld + f] * P[(int64_t)i * ldp + c];
            tot += term;
            if (c - i > D) hi += term;
            else if (c - i < -D) lo += term;
        }
        below += w * lo;
        above += w * hi;
        m1 += (double)c * (w * tot);
    }
    double* o = acc + (int64_t)(2 * D + 1) * stride + f;
    o[0] = first ? pk * below : o[0] + pk * below;
    o[stride] = first ? pk * above : o[stride] + pk * above;
    nm[f] = first ? pk * m1 : nm[f] + pk * m1;
}

// ---------------------------------------------------------------------------------------------------------------- finish
// nm[f] = sum_j j A[j][f] over an interior node's accumulated posterior; the root's launch also makes Z = sum_s A_root[s]
__global__ __launch_bounds__(256) void change_node_mean_kernel(const double* __restrict__ A, int jmax, int64_t ld, double* __restrict__ Z, double* __restrict__ nm) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    double z = 0.0, m = 0.0;
    for (int j = 0; j <= jmax; ++j) {
        const double p = A[(int64_t)j * ld + f];
        z += p;
        m += (double)j * p;
    }
    if (Z) Z[f] = z;
    nm[f] = m;
}

// Per column (blockIdx.x) and node (blockIdx.y): the band and the tails divided by Z in place, the mean, the first arg max
// over the band, and the two crossings of the CDF over (below, -D..D, above): -D-1 / D+1 where a crossing lies in a tail.
// The root and every node of a failed family: NaN and CAFE_CHANGE_NONE.
__global__ __launch_bounds__(256) void change_finish_kernel(double* __restrict__ acc, int D, int64_t ld, int64_t stride, const double* __restrict__ Z,
                                                            const double* __restrict__ nm, const int32_t* __restrict__ parent, int root, double level,
                                                            double* __restrict__ mean, int32_t* __restrict__ mode, int32_t* __restrict__ lo,
                                                            int32_t* __restrict__ hi) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= ld) return;
    const int v = blockIdx.y, nb = 2 * D + 1;
    double* a = acc + (int64_t)v * (nb + 2) * stride + f;
    const int64_t o = (int64_t)v * stride + f;
    const double z = Z[f], nan = __builtin_nan("");
    if (v == root || evidence_failed(z)) {
        for (int e = 0; e < nb + 2; ++e) a[(int64_t)e * stride] = nan;
        mean[o] = nan; mode[o] = CAFE_CHANGE_NONE; lo[o] = CAFE_CHANGE_NONE; hi[o] = CAFE_CHANGE_NONE;
        return;
    }
    const double tlo = 0.5 * (1.0 - level) * z, thi = (1.0 - 0.5 * (1.0 - level)) * z;
    const double below = a[(int64_t)nb * stride], above = a[(int64_t)(nb + 1) * stride];
    double cum = below, best = -1.0;
    int arg = -D, l = D + 1, h = D + 1;
    bool have_l = cum >= tlo, have_h = cum >= thi;
    if (have_l) l = -D - 1;
    if (have_h) h = -D - 1;
    for (int e = 0; e < nb; ++e) {
        const double p = a[(int64_t)e * stride];
        if (p > best) { best = p; arg = e - D; }
        cum += p;
        if (!have_l && cum >= tlo) { l = e - D; have_l = true; }
        if (!have_h && cum >= thi) { h = e - D; have_h = true; }
        a[(int64_t)e * stride] = p / z;
    }
    a[(int64_t)nb * stride] = below / z;
    a[(int64_t)(nb + 1) * stride] = above / z;
    mean[o] = nm[o] / z - nm[(int64_t)parent[v] * stride + f] / z;
    mode[o] = arg; lo[o] = l; hi[o] = h;
}

}  // namespace

int branch_change_impl(cafe_ctx* c, const cafe_params* pr, int32_t max_change, double level, const cafe_branch_change_out* out) {
    if (const int rc = check_call_args(c, "cafe_branch_change", pr, out)) return rc;
    if (!(level > 0.0 && level < 1.0)) { set_err(c, "cafe_branch_change: level must lie in (0, 1)"); return CAFE_ERR_ARGUMENT; }
    if (max_change < 0 || max_change > std::max(c->M, c->R)) {
        set_err(c, "cafe_branch_change: max_change must lie in 0..%d", std::max(c->M, c->R));
        return CAFE_ERR_ARGUMENT;
    }
    if (const int rc = check_model_args(c, "cafe_branch_change", pr)) return rc;
    PosteriorCall pc;
    if (const int rc = open_posterior_call(c, pr, &pc)) return rc;
    pc.timer.on = c->profile != 0;
    GemmTimer band_timer;
    band_timer.on = pc.timer.on;
    hipStream_t s = pc.s;
    UpPanels& up = pc.up;
    const int M = c->M, R = c->R, n = c->n_nodes, rows = c->N;      // a panel holds sizes 0..max(M, R)
    const int K = pc.K, nI = pc.nI, n_dev = pc.n_dev;
    const int D = max_change, nb = 2 * D + 1, na = nb + 2;          // per node: the band, below, above

    // workspace per column: B, F, O and the accumulation panel of every interior node, G and the tail panel, the band and
    // tails of every node, Z, the node mean numerators and the summaries
    const size_t dbl_per_col = (size_t)4 * nI * rows + 2 * (size_t)rows + (size_t)n * na + 1 + 2 * (size_t)n;
    const size_t per_col = dbl_per_col * sizeof(double) + (size_t)3 * n * sizeof(int32_t);
    int64_t cols = 0;
    if (const int rc = column_chunk(c, per_col, "cafe_branch_change: not enough device memory for the panels of " + std::to_string(nI) + " interior nodes", &cols))
        return rc;
    DevBuf wd, wi, wp;
    if (hipMalloc(&wd.p, dbl_per_col * cols * sizeof(double)) != hipSuccess || hipMalloc(&wi.p, (size_t)3 * n * cols * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&wp.p, (size_t)n * sizeof(int32_t)) != hipSuccess || alloc_constants(c, kNoPriorLogs, &pc) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "cafe_branch_change: cannot allocate the workspace (%lld columns)", (long long)cols);
        return CAFE_ERR_MEMORY;
    }
    HIP_TRY(c, hipMemsetAsync(wd.p, 0, dbl_per_col * cols * sizeof(double), s));
    const int64_t pstride = (int64_t)rows * cols;
    double* d_O = up.place(wd.p, nI, pstride);
    double* d_A = d_O + (int64_t)nI * pstride;
    double* d_G = d_A + (int64_t)nI * pstride;
    double* d_T = d_G + pstride;
    double* d_acc = d_T + pstride;                           // [node][2D + 3][cols]
    double* d_Z = d_acc + (int64_t)n * na * cols;
    double* d_nm = d_Z + cols;                               // [node][cols]
    double* d_mean = d_nm + (int64_t)n * cols;
    int32_t* d_mode = static_cast<int32_t*>(wi.p);
    int32_t* d_lo = d_mode + (int64_t)n * cols;
    int32_t* d_hi = d_lo + (int64_t)n * cols;
    int32_t* d_parent = static_cast<int32_t*>(wp.p);
    std::vector<int32_t> h_parent(n);
    for (int v = 0; v < n; ++v) h_parent[v] = v == c->root ? v : c->parent[v];
    HIP_TRY(c, hipMemcpyAsync(d_parent, h_parent.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    if (const int rc = upload_constants(c, pr, &pc)) return rc;

    std::vector<double> h_acc((size_t)n * na * cols), h_mean((size_t)n * cols), h_Z(cols);
    std::vector<int32_t> h_mode((size_t)n * cols), h_lo((size_t)n * cols), h_hi((size_t)n * cols);

    const std::vector<Branch> down = branches_down(c);
    for (int64_t f0 = 0; f0 < c->Fp; f0 += cols) {
        const int64_t ld = std::min<int64_t>(cols, c->Fp - f0);
        const unsigned gb = (unsigned)((ld + 255) / 256);
        for (int k = 0; k < K; ++k) {
            const double pk = pc.gamma ? pr->cat_probs[k] : 1.0;
            const int first = k == 0;
            if (const int rc = marginal_up_pass(c, up, k, f0, ld, s, pc.timer)) return rc;
            CAFE_LAUNCH(c, change_root_kernel, dim3(gb, (unsigned)((R + 1 + 15) / 16)), dim3(256), 0, s, up.panel(up.B, c->root), pc.prior, R, ld, up.panel(d_O, c->root),
                        up.panel(d_A, c->root), pk, first);
            for (const Branch& b : down) {
                const int v = b.v, np = b.np;
                double* acc_v = d_acc + (int64_t)v * na * cols;
                GemmParams g;
                if (const int rc = down_branch(c, up, d_O, d_G, b, k, pk, f0, ld, s, &g)) return rc;
                if (c->leaf_taxon[v] >= 0) {
                    CAFE_LAUNCH(c, change_leaf_kernel, dim3(gb), dim3(256), 0, s, d_G, np + 1, ld, leaf_matrix(c, v, k), c->pool.ld, leaf_counts(c, v, f0), up.err,
                                n_dev, M, D, acc_v, cols, d_nm + (int64_t)v * cols, pk, first);
                    continue;
                }
                g.out2 = up.panel(d_A, v); g.first = first;
                if (const int rc = launch_gemm<kDown>(c, g, false, s, pc.timer)) return rc;
                BandParams bp{};
                bp.Pt = g.Pt; bp.ldp = g.ldp; bp.G = d_G; bp.B = g.Bv; bp.ld = ld; bp.np = np; bp.M = M; bp.D = D;
                bp.ext = interior_extents(c, v, k); bp.acc = acc_v; bp.stride = cols; bp.pk = pk; bp.first = first;
                band_timer.mark(s);
                CAFE_LAUNCH(c, change_band_kernel, dim3((unsigned)(ld / kBandThreads), (unsigned)((nb + kBandD - 1) / kBandD)), dim3(kBandThreads), 0, s, bp);
                band_timer.mark(s);
                for (int m = 1; m <= 2; ++m) {               // above the band: i + D < j, then below it: i > j + D
                    TailGemm tg{};
                    tg.Pt = g.Pt; tg.ldp = g.ldp; tg.G = d_G; tg.Bv = g.Bv; tg.ld = ld; tg.nr = M + 1; tg.nk = np; tg.mask = m; tg.D = D; tg.out = d_T;
                    pc.timer.mark(s);
                    CAFE_LAUNCH(c, change_tail_gemm_kernel, dim3((unsigned)(ld / kNT), (unsigned)((tg.nr + kMT - 1) / kMT)), dim3(256), 0, s, tg);
                    pc.timer.mark(s);
                    const double left = std::max(0.0, (double)(m == 1 ? M - D : np - D));      // the mask's triangle
                    pc.timer.flops += left * left * (double)ld;
                    CAFE_LAUNCH(c, change_colsum_kernel, dim3(gb), dim3(256), 0, s, (const double*)d_T, M + 1, ld, acc_v + (int64_t)(nb + (m == 1 ? 1 : 0)) * cols, pk, first);
                }
            }
        }
        // ---- node means (the root's launch makes Z), then the summaries
        for (int v = 0; v < n; ++v) {
            if (c->leaf_taxon[v] >= 0) continue;
            const bool is_root = v == c->root;
            CAFE_LAUNCH(c, change_node_mean_kernel, dim3(gb), dim3(256), 0, s, (const double*)up.panel(d_A, v), is_root ? R : M, ld, is_root ? d_Z : nullptr,
                        d_nm + (int64_t)v * cols);
        }
        CAFE_LAUNCH(c, change_finish_kernel, dim3(gb, (unsigned)n), dim3(256), 0, s, d_acc, D, ld, cols, (const double*)d_Z, (const double*)d_nm, (const int32_t*)d_parent, c->root,
                    level, d_mean, d_mode, d_lo, d_hi);
        if (out->pmf) {
            HIP_TRY(c, hipMemcpyAsync(h_acc.data(), d_acc, sizeof(double) * (size_t)n * na * cols, hipMemcpyDeviceToHost, s));
        } else if (out->below || out->above) {               // the bands stay on the device: the two tails of every node
            for (int v = 0; v < n; ++v) {
                const size_t at = ((size_t)v * na + nb) * cols;
                HIP_TRY(c, hipMemcpyAsync(h_acc.data() + at, d_acc + at, sizeof(double) * 2 * (size_t)cols, hipMemcpyDeviceToHost, s));
            }
        }
        HIP_TRY(c, hipMemcpyAsync(h_mean.data(), d_mean, sizeof(double) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_mode.data(), d_mode, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_lo.data(), d_lo, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_hi.data(), d_hi, sizeof(int32_t) * (size_t)n * cols, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_Z.data(), d_Z, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for_each_family_of_chunk(c, f0, ld, [&](int64_t f, int64_t col) {
            const double z = h_Z[col];
            const bool bad = evidence_failed(z);
            if (out->log_evidence) out->log_evidence[f] = bad ? kNaN : std::log(z);
            if (out->failed) out->failed[f] = bad ? 1 : 0;
            for (int v = 0; v < n; ++v) {
                const size_t src = (size_t)v * cols + col, dst = (size_t)f * n + v;
                const double* a = h_acc.data() + (size_t)v * na * cols + col;
                if (out->pmf) for (int e = 0; e < nb; ++e) out->pmf[dst * nb + e] = a[(size_t)e * cols];
                if (out->below) out->below[dst] = a[(size_t)nb * cols];
                if (out->above) out->above[dst] = a[(size_t)(nb + 1) * cols];
                if (out->mean) out->mean[dst] = h_mean[src];
                if (out->mode) out->mode[dst] = h_mode[src];
                if (out->lo) out->lo[dst] = h_lo[src];
                if (out->hi) out->hi[dst] = h_hi[src];
            }
        });
    }
    close_posterior_call(c, &pc.timer);
    c->change_band_ms = band_timer.on ? band_timer.total_ms() : 0.0;
    return CAFE_OK;
}

}  // namespace cafe

extern "C" {

int cafe_branch_change(cafe_ctx* ctx, const cafe_params* params, int32_t max_change, double level, const cafe_branch_change_out* out) {
    return cafe::guarded_observed(ctx, "cafe_branch_change", [&] { return cafe::branch_change_impl(ctx, params, max_change, level, out); });
}

int cafe_debug_branch_change_band(cafe_ctx* ctx, double* ms) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    if (ms) *ms = ctx->change_band_ms;
    return CAFE_OK;
}

}
