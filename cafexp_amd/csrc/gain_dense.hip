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
// Plain fp64, no rescaling, by default.  A column's value is computed by the same operations in the same order wherever the
// column stands, so it depends on the family's counts and the rates only: not on its position, not on the batch cut.
//
// cafe_set_gain_scaling switches both entries to the SCALED mode ("scaled" below): every panel is held as mantissas and one
// int32 binary exponent per (node, column), B~_v[s][f] = B_v[s][f] 2^-E_v[f], E chosen so that the column's largest entry has
// binary exponent 0.  A power of two per column commutes with the GEMMs exactly, so both GEMM kernels run as they are and their
// outputs carry their inputs' exponents; the product, weights, root and output kernels have scaled twins.  Matrix entries stay
// plain fp64.
//
// cafe_gain_posterior_dense: the same up pass with the sum rule forced, then the other half of the sum-product on the panels it
// left -- by depth from the root a weights kernel, an MFMA GEMM over the matrices as stored (P^T), and the output kernels of
// the interior nodes and of the leaves ("down" below).  Both entries run gain_dense_impl.
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
    int32_t carry;                   // scaled: the F panel (an index) that the GEMM makes of this one and that carries its exponents, -1 at the root
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

// v *= f.  Track (the scaled kernels): the element is the pair (v, k) standing for v 2^(-512 k).  A non-zero factor below 2^-512
// is lifted by 2^512 before the multiplication and a non-zero product below 2^-512 after it, each counted in k, so a many-way
// product of factors each above 2^-1024 stays within 2^-1024 of the normal range while its exponent is still unknown.  Each is
// lifted ONCE: a product of two values just above 2^-512 can land in [2^-1024, 2^-1022) and lose up to two bits before its lift,
// and a factor below 2^-1024 (a denormal matrix entry, or a mantissa that far under its column's largest) stays below 2^-512
// after its lift, so the product under it can lose more.  Both need values more than 150 decimal orders under their column's
// largest or a denormal matrix entry.  The lifts are powers of two: where nothing was going to underflow the mantissa is the
// untracked product's.
constexpr double kGdTiny = 0x1p-512, kGdLift = 0x1p+512;
template <bool Track>
__device__ __forceinline__ void gain_dense_mul(double& v, int& k, double f) {
    if constexpr (Track) {
        if (f > 0.0 && f < kGdTiny) { f *= kGdLift; ++k; }
        v *= f;
        if (v > 0.0 && v < kGdTiny) { v *= kGdLift; ++k; }
    } else {
        v *= f;
    }
}

// v[j] *= the factor of every listed child at parent size i0 + j, children in list order: an interior child's F panel, a leaf's
// gather from its matrix (taps ascending; a missing cell exactly 1.0; a count past M 0).  The product kernel's body, and the
// sibling product of the down pass's weights.  Track: gain_dense_mul's lifts are counted in k[j]; an interior child's panel is then
// its mantissas, and the caller adds the child's column exponent.
template <bool Track = false>
__device__ __forceinline__ void gain_dense_times_children(const GainProdArgs& a, int child0, int n_children, int i0, int n, int64_t f, int64_t col,
                                                          double (&v)[kGdProdRows], int (&k)[kGdProdRows]) {
    for (int ci = 0; ci < n_children; ++ci) {
        const GainChild ch = a.children[child0 + ci];
        if (ch.taxon < 0) {
            const double* __restrict__ F = a.panels + ch.src + (int64_t)i0 * a.ld + f;
#pragma unroll
            for (int j = 0; j < kGdProdRows; ++j)
                if (j < n) gain_dense_mul<Track>(v[j], k[j], F[(int64_t)j * a.ld]);
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
                if (j < n) gain_dense_mul<Track>(v[j], k[j], in ? pc[j] : 0.0);
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
            for (int j = 0; j < kGdProdRows; ++j) gain_dense_mul<Track>(v[j], k[j], fac[j]);
        }
    }
}

// grid (column blocks of 256, row blocks of 16, nodes of the level); a thread owns one column and 16 sizes
__global__ __launch_bounds__(256) void gain_dense_product_kernel(const GainProdArgs a) {
    const GainProdOp op = a.ops[blockIdx.z];
    const int i0 = blockIdx.y * kGdProdRows;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 >= op.rows || f >= a.ncols) return;
    const int n = min(kGdProdRows, op.rows - i0);
    double v[kGdProdRows];
    int lifts[kGdProdRows];                            // (not read: the untracked product)
#pragma unroll
    for (int j = 0; j < kGdProdRows; ++j) v[j] = 1.0;
    gain_dense_times_children(a, op.child0, op.n_children, i0, n, f, a.col[f], v, lifts);
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

// 64 columns per block, the sizes dealt to four waves: t_j = log B[j][f] + logmass[j], then the maximum, or m + log sum exp(t - m).
// Scaled: B is the root's mantissas, so that value is the log of the scaled evidence Z~ -- kept in zt for the down pass -- and
// lnL = log Z~ + E_root ln 2 (-inf for a zero column, whose exponent is 0).
template <bool Scaled>
__device__ __forceinline__ void gain_dense_root(const GainRootArgs& a, double (*red)[64], const int32_t* exps, double* zt) {
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
    if (y != 0) return;
    const double z = a.sum_rule ? m + log((red[0][x] + red[1][x]) + (red[2][x] + red[3][x])) : m;
    if constexpr (Scaled) {
        zt[f] = z;
        a.out[f] = z + (double)exps[f] * 0.693147180559945309417;
    } else {
        a.out[f] = z;
    }
}

__global__ __launch_bounds__(256) void gain_dense_root_kernel(const GainRootArgs a) {
    __shared__ double red[4][64];
    gain_dense_root<false>(a, red, nullptr, nullptr);
}

// exps: the exponents of the root's panel
__global__ __launch_bounds__(256) void gain_scaled_root_kernel(const GainRootArgs a, const int32_t* exps, double* zt) {
    __shared__ double red[4][64];
    gain_dense_root<true>(a, red, exps, zt);
}

// ------------------------------------------------------------------------------------------------------- down: weights
// cafe_gain_posterior_dense goes on where the root kernel stops, by DEPTH from the root (a branch is ready when its parent's
// outside vector is).  w_u[s][f] = outside_parent[s][f] * prod_{siblings v != u} factor_v[s][f], s < rows(u): what the rest of
// the tree says of the parent's size s.  The root's outside vector is the mass.  The product kernel's layout and its factors.
struct GainWeightOp {
    int64_t dst;                     // w panel of the node (doubles from `panels`)
    int64_t outside;                 // the parent's outside panel; -1: the parent is the root, its outside vector is `mass`
    int32_t rows;                    // R + 1 under the root, M + 1 below
    int32_t child0, n_children;      // the siblings, in child order
    int32_t carry;                   // scaled: the node's outside panel (an index), which carries w's exponents; -1 for a leaf
};
struct GainWeightArgs {
    GainProdArgs p;                  // (its ops are not read)
    const GainWeightOp* ops;
    const double* mass;              // [R + 1] root_absent, (1 - root_absent) (double)(float)prior[j - 1]
};

// grid (column blocks of 256, row blocks of 16, nodes of the depth)
__global__ __launch_bounds__(256) void gain_posterior_dense_weights_kernel(const GainWeightArgs a) {
    const GainWeightOp op = a.ops[blockIdx.z];
    const int i0 = blockIdx.y * kGdProdRows;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 >= op.rows || f >= a.p.ncols) return;
    const int n = min(kGdProdRows, op.rows - i0);
    double v[kGdProdRows];
    int lifts[kGdProdRows];                            // (not read: the untracked product)
#pragma unroll
    for (int j = 0; j < kGdProdRows; ++j) v[j] = 0.0;
    if (op.outside < 0) {
#pragma unroll
        for (int j = 0; j < kGdProdRows; ++j)
            if (j < n) v[j] = a.mass[i0 + j];
    } else {
        const double* __restrict__ O = a.p.panels + op.outside + (int64_t)i0 * a.p.ld + f;
#pragma unroll
        for (int j = 0; j < kGdProdRows; ++j)
            if (j < n) v[j] = O[(int64_t)j * a.p.ld];
    }
    gain_dense_times_children(a.p, op.child0, op.n_children, i0, n, f, a.p.col[f], v, lifts);
    double* __restrict__ dst = a.p.panels + op.dst + (int64_t)i0 * a.p.ld + f;
#pragma unroll
    for (int j = 0; j < kGdProdRows; ++j)
        if (j < n) dst[(int64_t)j * a.p.ld] = v[j];
}

// --------------------------------------------------------------------------------------- scaled: product and weights
// The scaled twins of the product and the weights kernel.  The plain kernels give a thread 16 sizes of a column and their
// blocks along y never meet, so no column maximum exists there.  Here a workgroup owns 64 columns over ALL sizes of the node:
// lanes along f (a panel row is read and written 512 contiguous bytes at a time), the 16-size chunks dealt to the four waves --
// wave y takes the chunks y, y + 4, .. -- as the root kernel deals sizes.
//   pass 1  forms every element as (mantissa, lifts) with gain_dense_times_children<true> and keeps only the largest binary
//           exponent of the column, folded across the four waves through LDS
//   pass 2  forms the elements again (the inputs now come from L2) and stores them shifted by that exponent: the panel is
//           written once and no unscaled panel ever reaches memory
// The column's exponent is the sum of the exponents its factors carry (the interior children's; under the weights also the
// parent's outside vector's) plus the shift.  An all-zero column and a column holding a NaN or an infinity get exponent 0; the
// latter is stored as it is, unscaled.  Everything a column sees is its own: no value depends on the column's neighbours.
struct GainScaleArgs {
    int32_t* exps;                   // [panels][ld]: the exponents of the panel at `off` doubles from `panels` are exps + off / N
    int32_t N;
};

constexpr int kGdNoExp = INT32_MIN, kGdBadExp = INT32_MAX;    // an all-zero column; one holding a NaN or an infinity

// grid (column tiles of 64, nodes).  init(i0, n, v): the elements before the children are multiplied in, as mantissas of the
// exponent e0.
template <class Init>
__device__ __forceinline__ void gain_scaled_node(const GainProdArgs& a, const GainScaleArgs& sc, int (*red)[64], int child0, int n_children, int rows,
                                                 int64_t dst, int carry, int e0, Init init) {
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 64 + x, col = a.col[f];
    int ecol = e0;
    for (int ci = 0; ci < n_children; ++ci) {
        const GainChild ch = a.children[child0 + ci];
        if (ch.taxon < 0) ecol += sc.exps[ch.src / sc.N + f];
    }
    double v[kGdProdRows];
    int k[kGdProdRows];
    auto form = [&](int i0, int n) {
        init(i0, n, v);
#pragma unroll
        for (int j = 0; j < kGdProdRows; ++j) k[j] = 0;
        gain_dense_times_children<true>(a, child0, n_children, i0, n, f, col, v, k);
    };
    int best = kGdNoExp;
    for (int i0 = y * kGdProdRows; i0 < rows; i0 += 4 * kGdProdRows) {
        const int n = min(kGdProdRows, rows - i0);
        form(i0, n);
#pragma unroll
        for (int j = 0; j < kGdProdRows; ++j)
            if (j < n && v[j] != 0.0) best = max(best, isfinite(v[j]) ? ilogb(v[j]) - 512 * k[j] : kGdBadExp);
    }
    red[y][x] = best;
    __syncthreads();
    best = max(max(red[0][x], red[1][x]), max(red[2][x], red[3][x]));
    const int shift = (best == kGdNoExp || best == kGdBadExp) ? -ecol : best;
    for (int i0 = y * kGdProdRows; i0 < rows; i0 += 4 * kGdProdRows) {
        const int n = min(kGdProdRows, rows - i0);
        form(i0, n);
        double* __restrict__ out = a.panels + dst + (int64_t)i0 * a.ld + f;
#pragma unroll
        for (int j = 0; j < kGdProdRows; ++j)
            if (j < n) out[(int64_t)j * a.ld] = ldexp(v[j], -512 * k[j] - shift);
    }
    if (y != 0) return;
    sc.exps[dst / sc.N + f] = ecol + shift;
    if (carry >= 0) sc.exps[(int64_t)carry * a.ld + f] = ecol + shift;
}

__global__ __launch_bounds__(256) void gain_scaled_product_kernel(const GainProdArgs a, const GainScaleArgs sc) {
    __shared__ int red[4][64];
    const GainProdOp op = a.ops[blockIdx.y];
    gain_scaled_node(a, sc, red, op.child0, op.n_children, op.rows, op.dst, op.carry, 0, [](int, int, double (&v)[kGdProdRows]) {
#pragma unroll
        for (int j = 0; j < kGdProdRows; ++j) v[j] = 1.0;
    });
}

// under the root the outside vector is the plain mass, exponent 0
__global__ __launch_bounds__(256) void gain_scaled_weights_kernel(const GainWeightArgs a, const GainScaleArgs sc) {
    __shared__ int red[4][64];
    const GainWeightOp op = a.ops[blockIdx.y];
    const int64_t f = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const int e0 = op.outside < 0 ? 0 : sc.exps[op.outside / sc.N + f];
    gain_scaled_node(a.p, sc, red, op.child0, op.n_children, op.rows, op.dst, op.carry, e0, [&](int i0, int n, double (&v)[kGdProdRows]) {
        const double* __restrict__ O = op.outside < 0 ? a.mass + i0 : a.p.panels + op.outside + (int64_t)i0 * a.p.ld + f;
        const int64_t step = op.outside < 0 ? 1 : a.p.ld;
#pragma unroll
        for (int j = 0; j < kGdProdRows; ++j) v[j] = j < n ? O[j * step] : 0.0;
    });
}

// ----------------------------------------------------------------------------------------------- down: transposed GEMM
// outside_u[c][f] = sum_{s < rows(u)} P_u[s][c] w_u[s][f], c = 0..M: A[c][s] = Pt[c * ldp + s] is the matrix AS STORED, the
// contraction index contiguous.  The tile, the waves, the fragment maps, the two buffer pairs and the B staging are the up
// GEMM's; the A staging is its own.  Thread t loads four consecutive k of row t >> 2 (two aligned double2: ldp is even, K steps
// are multiples of 16), so four neighbouring lanes cover the 128 bytes of a row and a wave 16 rows.  The LDS tile stays
// k-major for the fragment maps, so the store is the transposing step: lane (row, q = t & 3) writes As[4 q + e][row], e = 0..3.
// With the plain k * 80 + row the four q of a half-wave would meet in the same banks (4 * 80 = 0 mod 32 doubles): the row
// index is XORed with q << 3, which sends the 8 rows x 4 q of a half-wave to 32 different doubles.  The swizzle is constant over
// the four k of a fragment step (k >> 2 = s4) and permutes rows inside aligned groups of 32, so a fragment read still finds
// 16 consecutive doubles per k, and its two k of a half-wave 16 doubles apart (80 = 16 mod 32): neither side serialises.
// The contraction length is the op's (R + 1 and M + 1 meet in one launch); every load is guarded, c <= M and s < rows(u).
struct GainGemmTOp {
    int64_t Pt, W, O;                // matrix (doubles from `mats`), w and outside panels (doubles from `panels`)
    int32_t nk;                      // contraction over s = 0..nk-1
    int32_t pad;
};
struct GainGemmTArgs {
    const GainGemmTOp* ops;
    const double* mats;
    double* panels;
    int64_t ld;
    int32_t nr, ldp;                 // rows c = 0..nr-1 of the outside panel
};

// One 64 x 128 tile of that product: acc = A[r0 .. r0 + 63][0 .. nk) X[0 .. nk)[c0 .. c0 + 127], the K loop of both kernels that
// contract over a matrix as stored.  Ends behind a barrier: the buffers are free for the caller's next tile.
typedef double gd4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void gain_dense_tile_t(double (*As)[kGdKT * kGdLdA], double (*Xs)[kGdKT * kGdLdX], const double* __restrict__ mat,
                                                  const double* __restrict__ X, int r0, int nr, int nk, int ldp, int64_t ld, int64_t c0, gd4 (&acc)[4][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int arow = tid >> 2, aq = tid & 3;           // A staging: row of the tile, quad of k
    const double* __restrict__ Pt = mat + (int64_t)(r0 + arow) * ldp;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (gd4){0.0, 0.0, 0.0, 0.0};
    double2 ra[2], rx[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = k0 + 4 * aq + 2 * h;                              // (even: k < nk <= ldp keeps k + 1 inside the row)
            double2 v = make_double2(0.0, 0.0);
            if (r0 + arow < nr && k < nk) {
                v = *reinterpret_cast<const double2*>(Pt + k);
                if (k + 1 >= nk) v.y = 0.0;
            }
            ra[h] = v;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + wave + 4 * u;
            rx[u] = k < nk ? *reinterpret_cast<const double2*>(X + (int64_t)k * ld + c0 + 2 * lane) : make_double2(0.0, 0.0);
        }
    };
    auto stage = [&](int buf) {
        const int col = arow ^ (aq << 3);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            As[buf][(4 * aq + 2 * h) * kGdLdA + col] = ra[h].x;
            As[buf][(4 * aq + 2 * h + 1) * kGdLdA + col] = ra[h].y;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) *reinterpret_cast<double2*>(&Xs[buf][(wave + 4 * u) * kGdLdX + 2 * lane]) = rx[u];
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
            for (int i = 0; i < 4; ++i) af[i] = As[buf][(4 * s4 + l4) * kGdLdA + ((16 * i + l15) ^ (s4 << 3))];
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
}

// grid (column tiles, row tiles of M + 1, interior non-root nodes of the depth)
__global__ __launch_bounds__(256) void gain_posterior_dense_gemm_t_kernel(const GainGemmTArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][kGdKT * kGdLdA];
    __shared__ __attribute__((aligned(16))) double Xs[2][kGdKT * kGdLdX];
    const GainGemmTOp op = a.ops[blockIdx.z];
    const int r0 = blockIdx.y * kGdMT, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4, nr = a.nr;
    const int64_t c0 = (int64_t)blockIdx.x * kGdCols, ld = a.ld;
    gd4 acc[4][2];
    gain_dense_tile_t(As, Xs, a.mats + op.Pt, a.panels + op.W, r0, nr, op.nk, a.ldp, ld, c0, acc);
    double* __restrict__ O = a.panels + op.O;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 16 * i + l4 + 4 * q;
                if (r < nr) O[(int64_t)r * ld + c0 + 32 * wave + 16 * j + l15] = acc[i][j][q];
            }
}

// ------------------------------------------------------------------------------------------------------- down: outputs
// Both output kernels: 64 columns per block, lanes along f, the sizes dealt to four waves and folded in a fixed order.
// res is [4][n_nodes][ld]: p_absent, mean, p_gain, p_loss; posterior, when asked for, [n_nodes][N][ld].  Everything / Z.
struct GainNodeOp {
    int64_t outside, B, W, Pt;       // interior: outside (-1: the root, `mass`), B, w (-1 at the root) panels, the matrix; leaf: W, Pt
    int32_t node;
    int32_t n;                       // interior: the node's sizes 0..n-1 (R + 1 at the root, M + 1 below)
    int32_t rows;                    // rows(u): the parent's sizes
    int32_t taxon;                   // leaf: its row of `counts`
};
struct GainOutArgs {
    const GainNodeOp* ops;
    const double* mats;
    const double* panels;
    const double* mass;
    const double* lnl;               // [ld] the root kernel's sum-rule lnL: Z = exp(lnl); scaled: its log Z~
    double* res;
    double* posterior;               // or nullptr
    const int64_t* col;
    const int32_t* counts;
    const double* err;
    int64_t counts_ld, ld;
    int32_t nn, N, M, ldp, n_dev, any_missing;
    int64_t root_B;                  // the root's panel (doubles from `panels`): scaled, where E_root stands
};

__device__ __forceinline__ double gain_dense_fold4(double (*red)[64], int x, int y, double v) {
    red[y][x] = v;
    __syncthreads();
    const double s = (red[0][x] + red[1][x]) + (red[2][x] + red[3][x]);
    __syncthreads();                                   // red is free again
    return s;
}

// Scaled: the operands are mantissas and Z is Z~, so a ratio is short of its value by 2^d, d = E_w(u) + E_u - E_root for every
// output of the node (outside_u carries w_u's exponent; a leaf's own vector is its taps, exponent 0; at the root d = 0).  The
// ratio is formed first and shifted by ldexp after: nothing goes through exp(lnl).  The ratio is a product of two mantissas, so
// where d is large and positive -- the outside vector and the node's own vector peak at sizes hundreds of binary orders apart --
// it can pass through the denormal range, or to 0 below 2^-1074, before the shift brings it back: such an entry is short of
// bits though its value is representable.  Shifting one operand first would keep it; no input of the tests reaches this.
template <bool Scaled>
__device__ __forceinline__ double gain_dense_shifted(double ratio, int d) {
    if constexpr (Scaled) return ldexp(ratio, d);
    return ratio;
}

// interior nodes, the root among them (its op has no w: p_gain and p_loss are NaN): posterior_u[c] = outside_u[c] B_u[c] / Z,
// p_gain = w[0] sum_{c >= 1} P[0][c] B[c] / Z (row 0 is Pt[c * ldp], wave-uniform), p_loss = B[0] sum_{s >= 1} w[s] P[s][0] / Z
// (column 0 is Pt[s]).  grid (cols / 64, interior nodes of the depth)
template <bool Scaled>
__device__ __forceinline__ void gain_posterior_dense_interior(const GainOutArgs& a, double (*red)[64], const int32_t* exps) {
    const GainNodeOp op = a.ops[blockIdx.y];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 64 + x, ld = a.ld;
    const bool root = op.W < 0;
    const double Z = exp(a.lnl[f]);
    int d = 0;
    if constexpr (Scaled)
        if (!root) d = exps[op.W / a.N + f] + exps[op.B / a.N + f] - exps[a.root_B / a.N + f];
    const double* __restrict__ B = a.panels + op.B + f;
    const double* __restrict__ O = a.panels + (root ? op.B : op.outside) + f;
    const double* __restrict__ W = a.panels + (root ? op.B : op.W) + f;
    const double* __restrict__ Pt = a.mats + op.Pt;
    double m = 0.0, g = 0.0, l = 0.0, p0 = 0.0;
    for (int c = y; c < a.N; c += 4) {
        double post = 0.0;
        if (c < op.n) {
            const double b = B[(int64_t)c * ld];
            post = gain_dense_shifted<Scaled>((root ? a.mass[c] : O[(int64_t)c * ld]) * b / Z, d);
            m = fma((double)c, post, m);
            if (!root && c >= 1) g = fma(Pt[(int64_t)c * a.ldp], b, g);
        }
        if (!root && c >= 1 && c < op.rows) l = fma(W[(int64_t)c * ld], Pt[c], l);
        if (c == 0) p0 = post;
        if (a.posterior) a.posterior[((int64_t)op.node * a.N + c) * ld + f] = post;
    }
    m = gain_dense_fold4(red, x, y, m);
    g = gain_dense_fold4(red, x, y, g);
    l = gain_dense_fold4(red, x, y, l);
    if (y != 0) return;
    const int64_t o = (int64_t)op.node * ld + f, k = (int64_t)a.nn * ld;
    a.res[o] = p0;
    a.res[o + k] = m;
    a.res[o + 2 * k] = root ? __builtin_nan("") : gain_dense_shifted<Scaled>(W[0] * g / Z, d);
    a.res[o + 3 * k] = root ? __builtin_nan("") : gain_dense_shifted<Scaled>(B[0] * l / Z, d);
}

__global__ __launch_bounds__(256) void gain_posterior_dense_interior_kernel(const GainOutArgs a) {
    __shared__ double red[4][64];
    gain_posterior_dense_interior<false>(a, red, nullptr);
}

__global__ __launch_bounds__(256) void gain_scaled_interior_kernel(const GainOutArgs a, const int32_t* exps) {
    __shared__ double red[4][64];
    gain_posterior_dense_interior<true>(a, red, exps);
}

// leaves, without a GEMM: L_u is non-zero at the taps of the observed count only, so outside_u is needed there only --
// sum_s w[s] Pt[c * ldp + s], a dot along a contiguous matrix column, the product kernel's gather turned round.  The four
// waves take a quarter of the parent's sizes each.  A MISSING leaf (L_u = 1 over 0..M; on a context created with missing cells)
// gets the full mat-vec from its own thread group instead: wave y the sizes c = y, y + 4, .., each a whole dot.  Its p_gain is
// w[0] (1 - P[0][0]) / Z.  A count past M made lnl -inf: nothing is read for it.  grid (cols / 64, leaves of the depth)
template <bool Scaled>
__device__ __forceinline__ void gain_posterior_dense_leaf(const GainOutArgs& a, double (*red)[64], const int32_t* exps) {
    const GainNodeOp op = a.ops[blockIdx.y];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * 64 + x, ld = a.ld;
    const double Z = exp(a.lnl[f]);
    int d = 0;
    if constexpr (Scaled) d = exps[op.W / a.N + f] - exps[a.root_B / a.N + f];
    const int64_t col = a.col[f];
    const int cnt = col >= 0 ? a.counts[(int64_t)op.taxon * a.counts_ld + col] : 0;
    const bool missing = count_is_missing(cnt), in = !missing && cnt <= a.M;
    const double* __restrict__ W = a.panels + op.W + f;
    const double* __restrict__ Pt = a.mats + op.Pt;
    const int chunk = (op.rows + 3) / 4, s_lo = y * chunk, s_hi = min(op.rows, s_lo + chunk);
    double* __restrict__ po = a.posterior ? a.posterior + (int64_t)op.node * a.N * ld + f : nullptr;
    if (po)
        for (int c = y; c < a.N; c += 4) po[(int64_t)c * ld] = 0.0;
    __syncthreads();                                   // the zeros stand before wave 0 writes the taps

    const int n_taps = a.err ? a.n_dev : 1, lo = a.err ? cnt - (a.n_dev - 1) / 2 : cnt;
    double p0 = 0.0, mean = 0.0, g = 0.0, L0 = missing ? 1.0 : 0.0;
    for (int t = 0; t < n_taps; ++t) {                 // taps ascending; those outside [0, M] are dropped
        const int c = lo + t;
        const bool ok = in && c >= 0 && c <= a.M;
        double part = 0.0;
        if (ok) {
            const double* __restrict__ pc = Pt + (int64_t)c * a.ldp;
            for (int s = s_lo; s < s_hi; ++s) part = fma(W[(int64_t)s * ld], pc[s], part);
        }
        const double dot = gain_dense_fold4(red, x, y, part);
        if (y == 0 && ok) {
            const double wt = a.err ? a.err[(int64_t)cnt * a.n_dev + t] : 1.0;
            const double post = gain_dense_shifted<Scaled>(dot * wt / Z, d);
            if (c == 0) { p0 = post; L0 = wt; }
            else g = fma(Pt[(int64_t)c * a.ldp], wt, g);
            mean = fma((double)c, post, mean);
            if (po) po[(int64_t)c * ld] = post;
        }
    }
    double part = 0.0;                                 // sum_{s >= 1} w[s] P[s][0]
    for (int s = max(s_lo, 1); s < s_hi; ++s) part = fma(W[(int64_t)s * ld], Pt[s], part);
    const double loss = gain_dense_fold4(red, x, y, part);

    if (a.any_missing) {                               // (kernel-uniform)
        double mm = 0.0;
        if (missing)
            for (int c = y; c <= a.M; c += 4) {
                const double* __restrict__ pc = Pt + (int64_t)c * a.ldp;
                double dot = 0.0;
                for (int s = 0; s < op.rows; ++s) dot = fma(W[(int64_t)s * ld], pc[s], dot);
                const double post = gain_dense_shifted<Scaled>(dot / Z, d);
                if (c == 0) p0 = post;
                mm = fma((double)c, post, mm);
                if (po) po[(int64_t)c * ld] = post;
            }
        mm = gain_dense_fold4(red, x, y, mm);
        if (missing) { mean = mm; g = 1.0 - Pt[0]; }
    }
    if (y != 0) return;
    const int64_t o = (int64_t)op.node * ld + f, k = (int64_t)a.nn * ld;
    a.res[o] = p0;
    a.res[o + k] = mean;
    a.res[o + 2 * k] = gain_dense_shifted<Scaled>(W[0] * g / Z, d);
    a.res[o + 3 * k] = gain_dense_shifted<Scaled>(L0 * loss / Z, d);
}

__global__ __launch_bounds__(256) void gain_posterior_dense_leaf_kernel(const GainOutArgs a) {
    __shared__ double red[4][64];
    gain_posterior_dense_leaf<false>(a, red, nullptr);
}

__global__ __launch_bounds__(256) void gain_scaled_leaf_kernel(const GainOutArgs a, const int32_t* exps) {
    __shared__ double red[4][64];
    gain_posterior_dense_leaf<true>(a, red, exps);
}

// -------------------------------------------------------------------------------------- down: leave-one-out predictive
// cafe_gain_leaf_predictive wants, for a leaf l, the whole of O_l = P_l^T w_l -- what the rest of the tree says of EVERY count the
// leaf might have shown -- but only six sums of each of its columns, so the transposed GEMM's tile runs with an epilogue that
// reduces the accumulators over c instead of storing them: no O panel ever reaches memory.  A workgroup owns (leaf, column tile)
// and walks the row tiles of 0..M in ascending order, re-reading its w tile (from L2) for each; the six sums of a column stay in
// the registers of the lanes that hold it.  An observed value y sees the true size c = y - half + t with weight err[y][t] (no
// error model: y = c, weight 1), so element O[c][f] goes, for the taps t ascending with 0 <= y <= M, as e = err[y][t] O[c][f] into
//   W += e, S1 += (y - x) e, S2 += (y - x)^2 e, and below, obs or above by y < x, y = x, y > x
// about the pivot x, the column's observed count (0 for a missing cell): a cell that sits where the model expects it keeps its
// variance.  A lane adds its 16 rows of a tile in ascending order; the four 16-lane groups that share a column meet at the end
// by two cross-lane exchanges, (g0 + g1) + (g2 + g3).  No atomics, and nothing of a column depends on its neighbours, its tile
// or the batch.  Every output is a ratio inside one column of one w panel: in the scaled mode the column's power of two
// cancels exactly and the kernel runs on the mantissas as it is.  res is [5][n_taxa][ld]: mean, sd, p_below, p_obs, p_above.
struct GainPredOp {
    int64_t Pt, W;                   // the leaf's matrix (doubles from `mats`), its w panel (doubles from `panels`)
    int32_t nk;                      // rows(l): the parent's sizes, the contraction
    int32_t taxon;                   // the leaf's row of `counts` and of res
};
struct GainPredArgs {
    const GainPredOp* ops;
    const double* mats;
    const double* panels;
    double* res;
    const int64_t* col;
    const int32_t* counts;
    const double* err;               // [(M+1)][n_dev] or nullptr
    int64_t counts_ld, ld;
    int32_t nr, ldp, n_dev, n_taxa;  // nr = M + 1
};

// grid (column tiles, leaves of the depth)
__global__ __launch_bounds__(256) void gain_predictive_dense_leaf_kernel(const GainPredArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][kGdKT * kGdLdA];
    __shared__ __attribute__((aligned(16))) double Xs[2][kGdKT * kGdLdX];
    const GainPredOp op = a.ops[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * kGdCols, ld = a.ld;
    const int nr = a.nr;
    int x[2];
    bool missing[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t col = a.col[c0 + 32 * wave + 16 * j + l15];
        const int cnt = col >= 0 ? a.counts[(int64_t)op.taxon * a.counts_ld + col] : 0;
        missing[j] = count_is_missing(cnt);
        x[j] = missing[j] ? 0 : cnt;
    }
    double sum[2][6];                                  // W, S1, S2, below, obs, above of the lane's two columns
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 6; ++k) sum[j][k] = 0.0;
    auto add = [&](int j, int y, double e) {           // the observed value y with mass e, about the pivot x[j]
        const double dy = (double)(y - x[j]);
        sum[j][0] += e;
        sum[j][1] = fma(dy, e, sum[j][1]);
        sum[j][2] = fma(dy * dy, e, sum[j][2]);
        sum[j][3] += y < x[j] ? e : 0.0;
        sum[j][4] += y == x[j] ? e : 0.0;
        sum[j][5] += y > x[j] ? e : 0.0;
    };
    for (int r0 = 0; r0 < nr; r0 += kGdMT) {
        gd4 acc[4][2];
        gain_dense_tile_t(As, Xs, a.mats + op.Pt, a.panels + op.W, r0, nr, op.nk, a.ldp, ld, c0, acc);
        if (a.err == nullptr) {                        // (kernel-uniform) no error model: y = c, weight 1 -- no tap loop, no load
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = r0 + 16 * i + l4 + 4 * q;
                    if (c >= nr) continue;
#pragma unroll
                    for (int j = 0; j < 2; ++j) add(j, c, acc[i][j][q]);
                }
            continue;
        }
        const int half = (a.n_dev - 1) / 2;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = r0 + 16 * i + l4 + 4 * q;
                if (c >= nr) continue;
                for (int t = 0; t < a.n_dev; ++t) {
                    const int y = c + half - t;
                    if (y < 0 || y >= nr) continue;
                    const double wt = a.err[(int64_t)y * a.n_dev + t];
#pragma unroll
                    for (int j = 0; j < 2; ++j) add(j, y, wt * acc[i][j][q]);
                }
            }
    }
    const double nan = __builtin_nan("");
    const int64_t plane = (int64_t)a.n_taxa * ld;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            sum[j][k] += __shfl_xor(sum[j][k], 16);
            sum[j][k] += __shfl_xor(sum[j][k], 32);
        }
        if (l4 != 0) continue;
        const double W = sum[j][0], m1 = sum[j][1] / W;
        const bool ok = W > 0.0 && isfinite(W);        // a predictive distribution without mass: NaN in all five
        double* __restrict__ out = a.res + (int64_t)op.taxon * ld + c0 + 32 * wave + 16 * j + l15;
        out[0] = ok ? (double)x[j] + m1 : nan;
        out[plane] = ok ? sqrt(fmax(sum[j][2] / W - m1 * m1, 0.0)) : nan;
        out[2 * plane] = ok && !missing[j] ? sum[j][3] / W : nan;
        out[3 * plane] = ok && !missing[j] ? sum[j][4] / W : nan;
        out[4 * plane] = ok && !missing[j] ? sum[j][5] / W : nan;
    }
}

// ------------------------------------------------------------------------------------- down: sizes, intervals, change
#include "gain_marginal_kernel.h"

// ---------------------------------------------------------------------------------------------------------------- host
enum { kGdBuild = 0, kGdProduct = 1, kGdGemm = 2, kGdRoot = 3, kGdWeights = 4, kGdGemmT = 5, kGdInterior = 6, kGdLeaf = 7, kGdPredict = 8, kGdKinds = 9 };

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
    void collect(double* ms) const {                   // ms[kind] += its launches
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

// The staging of one batch of the down pass's outputs and the way back to the caller's arrays
struct GainDownHost {
    const cafe_gain_posterior_out* out;
    std::vector<double> res, posterior;                // [4][n_nodes][nb], [n_nodes][N][nb]

    void collect(int64_t b0, int64_t nb, int nn, int N, const double* lnl) const {
        double* const dst[4] = {out->p_absent, out->mean, out->p_gain, out->p_loss};
        for (int64_t b = 0; b < nb; ++b) {
            if (!std::isfinite(lnl[b])) continue;      // the entry keeps its NaN
            for (int k = 0; k < 4; ++k)
                for (int v = 0; v < nn; ++v) dst[k][(b0 + b) * nn + v] = res[((size_t)k * nn + v) * nb + b];
            if (!out->posterior) continue;
            double* po = out->posterior + (b0 + b) * nn * N;
            for (int64_t i = 0; i < (int64_t)nn * N; ++i) po[i] = posterior[(size_t)i * nb + b];
        }
    }
};

// The same for cafe_gain_leaf_predictive: five numbers per (entry, taxon)
struct GainPredictHost {
    const cafe_gain_leaf_predictive_out* out;
    std::vector<double> res;                           // [5][n_taxa][nb]

    void collect(int64_t b0, int64_t nb, int T, const double* lnl) const {
        double* const dst[5] = {out->mean, out->sd, out->p_below, out->p_obs, out->p_above};
        for (int64_t b = 0; b < nb; ++b) {
            if (!std::isfinite(lnl[b])) continue;      // the entry keeps its NaN
            for (int k = 0; k < 5; ++k)
                for (int t = 0; dst[k] && t < T; ++t) dst[k][(b0 + b) * T + t] = res[((size_t)k * T + t) * nb + b];
        }
    }
};

// The same for cafe_gain_marginal_dense: four doubles and three integers per (entry, node)
struct GainMarginalHost {
    const cafe_gain_marginal_out* out;
    double level;
    std::vector<double> res;                           // [4][n_nodes][nb]: mean, p_increase, p_decrease, p_same
    std::vector<int32_t> ires;                         // [3][n_nodes][nb]: mode, lo, hi

    void collect(int64_t b0, int64_t nb, int nn, const double* lnl) const {
        double* const dst[4] = {out->mean, out->p_increase, out->p_decrease, out->p_same};
        int32_t* const idst[3] = {out->mode, out->lo, out->hi};
        for (int64_t b = 0; b < nb; ++b) {
            if (!std::isfinite(lnl[b])) continue;      // the entry keeps its NaN and -1
            for (int v = 0; v < nn; ++v) {
                for (int k = 0; k < 4; ++k) dst[k][(b0 + b) * nn + v] = res[((size_t)k * nn + v) * nb + b];
                for (int k = 0; k < 3; ++k) idst[k][(b0 + b) * nn + v] = ires[((size_t)k * nn + v) * nb + b];
            }
        }
    }
};

// All four entries: the planning (keys, levels, op tables, workspace), the up pass launch for launch, and -- with `down`, the
// posterior entry, or `pred`, the predictive one -- the sum rule forced at the root, the plan and the launches of the down pass
// behind the root kernel.  Both walk the depths with the weights kernel and the transposed GEMM of the interior nodes; `down` adds
// the output kernels of every node, `pred` the fused kernel of the depth's leaves.  `marg`, the marginal entry, walks them with the
// weights kernel, the SPLIT transposed GEMM in the other one's place, and the summary kernels of every node.
int gain_dense_impl(cafe_ctx* c, const char* who, const cafe_params* pr, const double* lam, const double* mus, const double* nus, double root_absent,
                    int64_t n, const int64_t* family, double* family_lnl, GainDownHost* down, GainPredictHost* pred = nullptr, GainMarginalHost* marg = nullptr) {
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
    const bool scaled = c->gain_scaling != 0;          // cafe_set_gain_scaling: the scaled twins of every kernel but the build and the GEMMs

    // ---- what the host decides alone: an invalid rate set is -inf in every entry, a NaN lambda that passes the rule NaN
    c->last.state = LastCall::kNone;                   // cafe_family_results is not meaningful after this call
    const bool walk = down || pred || marg;            // the down pass is planned and run
    const int T = c->n_taxa;
    double ms[kGdKinds] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, flops = 0.0;
    if (down) {
        std::copy(ms, ms + 8, c->gain_dense_posterior_ms);
        c->gain_dense_posterior_flops = 0.0;
    } else if (pred) {
        std::copy(ms, ms + 7, c->gain_predictive_ms);
        c->gain_predictive_flops = 0.0;
    } else if (marg) {
        std::copy(ms, ms + 9, c->gain_marginal_ms);
        c->gain_marginal_flops = 0.0;
    } else {
        std::copy(ms, ms + 4, c->gain_dense_ms);
        c->gain_dense_flops = 0.0;
    }
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

    // ---- the down pass: the nodes by depth (breadth first: parents in front of their children), an outside panel per interior
    // non-root node behind the up pass's panels, the w panels of the widest depth behind those
    std::vector<int> depth(nn, 0), by_depth{c->root}, depth_off{0}, oidx(nn, -1), widx(nn, -1);
    int n_down = 0, n_depths = 0;
    const bool want_posterior = down && down->out->posterior;
    if (walk) {
        int n_out = 0, widest = 0;
        for (size_t at = 0; at < by_depth.size(); ++at)
            for (int ch : c->children[by_depth[at]]) { depth[ch] = depth[by_depth[at]] + 1; by_depth.push_back(ch); }
        for (size_t at = 1; at <= by_depth.size(); ++at) {
            if (at < by_depth.size() && depth[by_depth[at]] == depth[by_depth[at - 1]]) continue;
            widest = std::max(widest, (int)at - depth_off.back());
            depth_off.push_back((int)at);
        }
        n_depths = (int)depth_off.size() - 1;
        for (int u : by_depth)
            if (u != c->root && c->leaf_taxon[u] < 0) oidx[u] = n_pan + n_out++;
        for (int d = 1; d < n_depths; ++d)
            for (int k = depth_off[d]; k < depth_off[d + 1]; ++k) widx[by_depth[k]] = n_pan + n_out + (k - depth_off[d]);
        n_down = n_out + widest;
    }

    // ---- columns per batch: the matrices stand once, a batch adds its panels
    const int split_tiles = (M + kGdMT) / kGdMT;       // row tiles of the split GEMM: its partials are [n_nodes][tiles][3][ld]
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t fixed_bytes = sizeof(double) * (size_t)mat_stride * n_keys + ((size_t)64 << 10) + sizeof(GainChild) * (size_t)nn +
                               sizeof(GainProdOp) * (size_t)nn + sizeof(GainGemmOp) * (size_t)nn + sizeof(SlotParamGain) * (size_t)n_keys +
                               sizeof(double) * ((size_t)R + 1 + (size_t)(M + 1) * c->n_dev) +
                               (walk ? (sizeof(GainChild) + sizeof(GainWeightOp) + sizeof(GainGemmTOp) + sizeof(GainNodeOp) + sizeof(GainPredOp) + sizeof(GainSplitOp)) * (size_t)nn + sizeof(double) * ((size_t)R + 1) : 0);
    const size_t column_bytes = sizeof(double) * (size_t)n_pan * N + sizeof(int64_t) + sizeof(double) +
                                (walk ? sizeof(double) * ((size_t)n_down * N + (pred ? 5 * (size_t)T : 4 * (size_t)nn) + (want_posterior ? (size_t)nn * N : 0)) : 0) +
                                (marg ? (sizeof(double) * 3 * (size_t)split_tiles + sizeof(int32_t) * 3) * (size_t)nn : 0) +     // the split's partials, the integers
                                (scaled ? sizeof(int32_t) * (size_t)(n_pan + n_down) + sizeof(double) : 0);     // the exponents, log Z~
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
            po.carry = fidx[u];
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
    // the down pass's tables, depth by depth: the weights of every node, the transposed GEMM and the outputs of the interior ones
    // (depth 0: the root's outputs alone), the outputs of the leaves
    std::vector<GainWeightOp> weight_ops;
    std::vector<GainGemmTOp> gemmt_ops;
    std::vector<GainNodeOp> int_ops, leaf_ops;
    std::vector<GainPredOp> pred_ops;                  // (a leaf has an entry in both leaf tables: leaf_off serves both)
    std::vector<GainSplitOp> split_ops;                // (beside gemmt_ops entry for entry: gemmt_off serves both)
    std::vector<int> weight_off{0}, gemmt_off{0}, int_off{0}, leaf_off{0}, weight_rows;
    for (int d = 0; d < n_depths; ++d) {
        int w_rows = 0;
        for (int k = depth_off[d]; k < depth_off[d + 1]; ++k) {
            const int u = by_depth[k], p = c->parent[u];
            if (u == c->root) {
                int_ops.push_back({-1, bidx[u] * pan_stride, -1, 0, u, R + 1, 0, -1});
                continue;
            }
            const int rows = (p == c->root ? R : M) + 1;
            GainWeightOp wo{widx[u] * pan_stride, p == c->root ? -1 : oidx[p] * pan_stride, rows, (int32_t)children.size(), 0, oidx[u]};
            for (int sib : c->children[p]) {
                if (sib == u) continue;
                const bool leaf = c->leaf_taxon[sib] >= 0;
                children.push_back({leaf ? node_key[sib] * mat_stride : fidx[sib] * pan_stride, leaf ? c->leaf_taxon[sib] : -1, 0});
            }
            wo.n_children = (int32_t)children.size() - wo.child0;
            weight_ops.push_back(wo);
            w_rows = std::max(w_rows, rows);
            if (c->leaf_taxon[u] >= 0) {
                leaf_ops.push_back({-1, -1, widx[u] * pan_stride, node_key[u] * mat_stride, u, M + 1, rows, c->leaf_taxon[u]});
                pred_ops.push_back({node_key[u] * mat_stride, widx[u] * pan_stride, rows, c->leaf_taxon[u]});
                continue;
            }
            gemmt_ops.push_back({node_key[u] * mat_stride, widx[u] * pan_stride, oidx[u] * pan_stride, rows, 0});
            split_ops.push_back({node_key[u] * mat_stride, widx[u] * pan_stride, oidx[u] * pan_stride, bidx[u] * pan_stride, rows, u});
            int_ops.push_back({oidx[u] * pan_stride, bidx[u] * pan_stride, widx[u] * pan_stride, node_key[u] * mat_stride, u, M + 1, rows, -1});
        }
        weight_off.push_back((int)weight_ops.size()); gemmt_off.push_back((int)gemmt_ops.size());
        int_off.push_back((int)int_ops.size()); leaf_off.push_back((int)leaf_ops.size());
        weight_rows.push_back(w_rows);
    }
    std::vector<double> mass;                          // the root's outside vector, beside logmass
    if (walk) {
        mass.resize((size_t)R + 1);
        mass[0] = root_absent;
        for (int j = 1; j <= R; ++j) mass[j] = (1.0 - root_absent) * (double)pr->prior[j - 1];
    }

    std::vector<double> reals((size_t)R + 1 + (size_t)(M + 1) * c->n_dev);  // log mass of the root sizes, error model
    reals[0] = std::log(root_absent);
    for (int j = 0; j < R; ++j) reals[j + 1] = std::log1p(-root_absent) + std::log((double)pr->prior[j]);    // compute() returns float
    if (c->n_dev > 0) std::memcpy(reals.data() + R + 1, pr->error_model, sizeof(double) * (size_t)(M + 1) * c->n_dev);

    std::vector<char> blob;
    const size_t o_children = put(blob, children), o_prod = put(blob, prod_ops), o_gemm = put(blob, gemm_ops), o_slots = put(blob, slots),
                 o_reals = put(blob, reals), o_weight = put(blob, weight_ops), o_gemmt = put(blob, gemmt_ops), o_int = put(blob, int_ops),
                 o_leaf = put(blob, leaf_ops), o_pred = put(blob, pred_ops), o_split = put(blob, split_ops), o_mass = put(blob, mass);
    const size_t o_col = family_align_up(blob.size()), o_out = o_col + family_align_up(sizeof(int64_t) * ld),
                 o_mats = o_out + family_align_up(sizeof(double) * ld), o_pan = o_mats + family_align_up(sizeof(double) * (size_t)mat_stride * n_keys),
                 o_res = o_pan + sizeof(double) * (size_t)pan_stride * (n_pan + n_down),
                 o_post = o_res + sizeof(double) * (down || marg ? 4 * (size_t)nn : pred ? 5 * (size_t)T : 0) * ld,
                 o_parts = o_post + (want_posterior ? sizeof(double) * (size_t)nn * N * ld : 0),
                 o_ires = o_parts + (marg ? sizeof(double) * 3 * (size_t)split_tiles * nn * ld : 0),
                 o_exps = o_ires + (marg ? family_align_up(sizeof(int32_t) * 3 * (size_t)nn * ld) : 0),
                 o_zt = o_exps + (scaled ? family_align_up(sizeof(int32_t) * (size_t)(n_pan + n_down) * ld) : 0),
                 need = o_zt + (scaled ? sizeof(double) * ld : 0);
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
    GainRootArgs ra{panels + bidx[c->root] * pan_stride, d_reals, reinterpret_cast<double*>(base + o_out), ld, R,
                    walk || c->root_rule == CAFE_ROOT_SUM ? 1 : 0};
    GainWeightArgs wa{pa, reinterpret_cast<const GainWeightOp*>(base + o_weight), reinterpret_cast<const double*>(base + o_mass)};
    GainGemmTArgs ta{reinterpret_cast<const GainGemmTOp*>(base + o_gemmt), mats, panels, ld, M + 1, ldp};
    GainOutArgs oa{};
    oa.mats = mats; oa.panels = panels; oa.mass = wa.mass; oa.lnl = ra.out;
    oa.res = reinterpret_cast<double*>(base + o_res); oa.posterior = want_posterior ? reinterpret_cast<double*>(base + o_post) : nullptr;
    oa.col = pa.col; oa.counts = pa.counts; oa.err = pa.err; oa.counts_ld = pa.counts_ld; oa.ld = ld;
    oa.nn = nn; oa.N = N; oa.M = M; oa.ldp = ldp; oa.n_dev = c->n_dev; oa.any_missing = c->has_missing ? 1 : 0;
    oa.root_B = bidx[c->root] * pan_stride;
    GainPredArgs qa{reinterpret_cast<const GainPredOp*>(base + o_pred), mats, panels, oa.res, pa.col, pa.counts, pa.err, pa.counts_ld, ld, M + 1, ldp, c->n_dev, T};
    const GainScaleArgs sa{reinterpret_cast<int32_t*>(base + o_exps), N};
    const int32_t* root_exps = sa.exps + bidx[c->root] * ld;
    double* zt = reinterpret_cast<double*>(base + o_zt);
    if (scaled) oa.lnl = zt;                           // the outputs divide by Z~ = exp(log Z~)
    if (down) {
        down->res.resize(4 * (size_t)nn * entries);
        if (want_posterior) down->posterior.resize((size_t)nn * N * entries);
    }
    if (pred) pred->res.resize(5 * (size_t)T * entries);
    GainSplitArgs xa{reinterpret_cast<const GainSplitOp*>(base + o_split), mats, panels, reinterpret_cast<double*>(base + o_parts), ld, M + 1, ldp};
    GainSummaryArgs ya{oa, xa.parts, reinterpret_cast<int32_t*>(base + o_ires), marg ? marg->level : 0.0, split_tiles};
    if (marg) {
        marg->res.resize(4 * (size_t)nn * entries);
        marg->ires.resize(3 * (size_t)nn * entries);
    }

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
            if (scaled)
                CAFE_LAUNCH(c, gain_scaled_product_kernel, dim3((unsigned)(cols / 64), (unsigned)np), dim3(256), 0, s, p, sa);
            else
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
                flops += 2.0 * round_up(gemm_ops[k].nr, kGdMT) * (double)round_up(M + 1, kGdKT) * (double)cols;
        }
        timer.mark(kGdRoot, s);
        if (scaled)
            CAFE_LAUNCH(c, gain_scaled_root_kernel, dim3((unsigned)(cols / 64)), dim3(256), 0, s, ra, root_exps, zt);
        else
            CAFE_LAUNCH(c, gain_dense_root_kernel, dim3((unsigned)(cols / 64)), dim3(256), 0, s, ra);
        timer.mark(kGdRoot, s);
        HIP_TRY(c, hipMemcpyAsync(res.data(), base + o_out, sizeof(double) * nb, hipMemcpyDeviceToHost, s));
        for (int d = 0; d < n_depths; ++d) {           // the down pass: every B and F panel of the batch is still in place
            const int nw = weight_off[d + 1] - weight_off[d], nt = gemmt_off[d + 1] - gemmt_off[d], ni = int_off[d + 1] - int_off[d],
                      nl = leaf_off[d + 1] - leaf_off[d];
            if (nw > 0) {
                GainWeightArgs w = wa;
                w.ops += weight_off[d];
                w.p.ncols = cols;
                timer.mark(kGdWeights, s);
                if (scaled)
                    CAFE_LAUNCH(c, gain_scaled_weights_kernel, dim3((unsigned)(cols / 64), (unsigned)nw), dim3(256), 0, s, w, sa);
                else
                    CAFE_LAUNCH(c, gain_posterior_dense_weights_kernel,
                                dim3((unsigned)((cols + 255) / 256), (unsigned)((weight_rows[d] + kGdProdRows - 1) / kGdProdRows), (unsigned)nw), dim3(256), 0, s, w);
                timer.mark(kGdWeights, s);
            }
            if (nt > 0 && marg) {                      // the split GEMM: the outside panels and the three sums of every branch
                GainSplitArgs x = xa;
                x.ops += gemmt_off[d];
                timer.mark(kGdGemmT, s);
                CAFE_LAUNCH(c, gain_marginal_dense_split_kernel, dim3(tiles, (unsigned)split_tiles, (unsigned)nt), dim3(256), 0, s, x);
                timer.mark(kGdGemmT, s);
                for (int k = gemmt_off[d]; k < gemmt_off[d + 1]; ++k)
                    for (int r0 = 0; r0 <= M; r0 += kGdMT) {               // the K tiles both phases issue, the masked repeats among them
                        const int k_end = round_up(split_ops[k].nk, kGdKT);
                        flops += 2.0 * kGdMT * (double)(gain_marginal_phase1_end(r0, split_ops[k].nk) + std::max(0, k_end - r0)) * (double)cols;
                    }
            } else if (nt > 0) {
                GainGemmTArgs t = ta;
                t.ops += gemmt_off[d];
                timer.mark(kGdGemmT, s);
                CAFE_LAUNCH(c, gain_posterior_dense_gemm_t_kernel, dim3(tiles, (unsigned)((M + kGdMT) / kGdMT), (unsigned)nt), dim3(256), 0, s, t);
                timer.mark(kGdGemmT, s);
                for (int k = gemmt_off[d]; k < gemmt_off[d + 1]; ++k)
                    flops += 2.0 * round_up(M + 1, kGdMT) * (double)round_up(gemmt_ops[k].nk, kGdKT) * (double)cols;
            }
            if (pred) {                                // the leaves' six sums straight from the MFMA accumulators; no other output
                if (nl == 0) continue;
                GainPredArgs q = qa;
                q.ops += leaf_off[d];
                timer.mark(kGdPredict, s);
                CAFE_LAUNCH(c, gain_predictive_dense_leaf_kernel, dim3(tiles, (unsigned)nl), dim3(256), 0, s, q);
                timer.mark(kGdPredict, s);
                for (int k = leaf_off[d]; k < leaf_off[d + 1]; ++k)
                    flops += 2.0 * round_up(M + 1, kGdMT) * (double)round_up(pred_ops[k].nk, kGdKT) * (double)cols;
                continue;
            }
            if (marg) {                                // the summaries: nothing of a posterior is stored
                GainSummaryArgs y = ya;
                if (ni > 0) {
                    y.o.ops = reinterpret_cast<const GainNodeOp*>(base + o_int) + int_off[d];
                    timer.mark(kGdInterior, s);
                    if (scaled)
                        CAFE_LAUNCH(c, gain_marginal_scaled_interior_kernel, dim3((unsigned)(cols / 64), (unsigned)ni), dim3(256), 0, s, y, (const int32_t*)sa.exps);
                    else
                        CAFE_LAUNCH(c, gain_marginal_dense_interior_kernel, dim3((unsigned)(cols / 64), (unsigned)ni), dim3(256), 0, s, y);
                    timer.mark(kGdInterior, s);
                }
                if (nl > 0) {
                    y.o.ops = reinterpret_cast<const GainNodeOp*>(base + o_leaf) + leaf_off[d];
                    timer.mark(kGdLeaf, s);
                    if (scaled)
                        CAFE_LAUNCH(c, gain_marginal_scaled_leaf_kernel, dim3((unsigned)(cols / 64), (unsigned)nl), dim3(256), 0, s, y, (const int32_t*)sa.exps);
                    else
                        CAFE_LAUNCH(c, gain_marginal_dense_leaf_kernel, dim3((unsigned)(cols / 64), (unsigned)nl), dim3(256), 0, s, y);
                    timer.mark(kGdLeaf, s);
                }
                continue;
            }
            GainOutArgs o = oa;
            if (ni > 0) {
                o.ops = reinterpret_cast<const GainNodeOp*>(base + o_int) + int_off[d];
                timer.mark(kGdInterior, s);
                if (scaled)
                    CAFE_LAUNCH(c, gain_scaled_interior_kernel, dim3((unsigned)(cols / 64), (unsigned)ni), dim3(256), 0, s, o, (const int32_t*)sa.exps);
                else
                    CAFE_LAUNCH(c, gain_posterior_dense_interior_kernel, dim3((unsigned)(cols / 64), (unsigned)ni), dim3(256), 0, s, o);
                timer.mark(kGdInterior, s);
            }
            if (nl > 0) {
                o.ops = reinterpret_cast<const GainNodeOp*>(base + o_leaf) + leaf_off[d];
                timer.mark(kGdLeaf, s);
                if (scaled)
                    CAFE_LAUNCH(c, gain_scaled_leaf_kernel, dim3((unsigned)(cols / 64), (unsigned)nl), dim3(256), 0, s, o, (const int32_t*)sa.exps);
                else
                    CAFE_LAUNCH(c, gain_posterior_dense_leaf_kernel, dim3((unsigned)(cols / 64), (unsigned)nl), dim3(256), 0, s, o);
                timer.mark(kGdLeaf, s);
            }
        }
        if (down) {                                    // [rows][ld] on the device, [rows][nb] on the host
            HIP_TRY(c, hipMemcpy2DAsync(down->res.data(), sizeof(double) * nb, oa.res, sizeof(double) * ld, sizeof(double) * nb, 4 * (size_t)nn,
                                        hipMemcpyDeviceToHost, s));
            if (want_posterior)
                HIP_TRY(c, hipMemcpy2DAsync(down->posterior.data(), sizeof(double) * nb, oa.posterior, sizeof(double) * ld, sizeof(double) * nb, (size_t)nn * N,
                                            hipMemcpyDeviceToHost, s));
        }
        if (pred)
            HIP_TRY(c, hipMemcpy2DAsync(pred->res.data(), sizeof(double) * nb, oa.res, sizeof(double) * ld, sizeof(double) * nb, 5 * (size_t)T,
                                        hipMemcpyDeviceToHost, s));
        if (marg) {
            HIP_TRY(c, hipMemcpy2DAsync(marg->res.data(), sizeof(double) * nb, oa.res, sizeof(double) * ld, sizeof(double) * nb, 4 * (size_t)nn,
                                        hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpy2DAsync(marg->ires.data(), sizeof(int32_t) * nb, ya.ires, sizeof(int32_t) * ld, sizeof(int32_t) * nb, 3 * (size_t)nn,
                                        hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(c, hipStreamSynchronize(s));            // the host tables of this batch go out of use
        std::copy(res.begin(), res.begin() + nb, family_lnl + b0);
        if (down) down->collect(b0, nb, nn, N, res.data());
        if (pred) pred->collect(b0, nb, T, res.data());
        if (marg) marg->collect(b0, nb, nn, res.data());
    }
    timer.collect(ms);
    if (pred) {
        ms[6] = ms[kGdPredict];                        // build, product, GEMM, root, weights, transposed GEMM, fused leaf
        std::copy(ms, ms + 7, c->gain_predictive_ms);
        c->gain_predictive_flops = flops;
        return CAFE_OK;
    }
    if (marg) {                                        // the posterior entry's eight, the split GEMM sixth; then their total
        ms[8] = 0.0;
        for (int k = 0; k < 8; ++k) ms[8] += ms[k];
        std::copy(ms, ms + 9, c->gain_marginal_ms);
        c->gain_marginal_flops = flops;
        return CAFE_OK;
    }
    std::copy(ms, ms + (down ? 8 : 4), down ? c->gain_dense_posterior_ms : c->gain_dense_ms);
    (down ? c->gain_dense_posterior_flops : c->gain_dense_flops) = flops;
    return CAFE_OK;
}

}  // namespace
}  // namespace cafe

int cafe_score_gain(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent, int64_t n,
                    const int64_t* family, double* family_lnl) {
    const int rc = cafe::guarded(ctx, "cafe_score_gain",
                                 [&] { return cafe::gain_dense_impl(ctx, "cafe_score_gain", params, lambdas, mus, nus, root_absent, n, family, family_lnl, nullptr); });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

int cafe_set_gain_scaling(cafe_ctx* ctx, int on) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    ctx->gain_scaling = on != 0;
    return CAFE_OK;
}

int cafe_debug_gain_dense(cafe_ctx* ctx, double ms[4], double* flops) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    for (int k = 0; ms && k < 4; ++k) ms[k] = ctx->gain_dense_ms[k];
    if (flops) *flops = ctx->gain_dense_flops;
    return CAFE_OK;
}

int cafe_gain_posterior_dense(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent,
                              int64_t n, const int64_t* family, const cafe_gain_posterior_out* out) {
    const char* const who = "cafe_gain_posterior_dense";
    const int rc = cafe::guarded(ctx, who, [&] {
        if (!out || (n > 0 && (!out->p_absent || !out->mean || !out->p_gain || !out->p_loss))) {
            cafe::set_err(ctx, "%s: out with p_absent, mean, p_gain and p_loss is required", who);
            return (int)CAFE_ERR_ARGUMENT;
        }
        std::vector<double> own_lnl;
        double* lnl = out->lnl;
        if (!lnl && n > 0) { own_lnl.resize((size_t)n); lnl = own_lnl.data(); }
        if (n > 0) {                                   // what no finite lnl replaces
            const size_t nodes = (size_t)n * ctx->n_nodes;
            const double nan = std::numeric_limits<double>::quiet_NaN();
            for (double* p : {out->p_absent, out->mean, out->p_gain, out->p_loss}) std::fill(p, p + nodes, nan);
            if (out->posterior) std::fill(out->posterior, out->posterior + nodes * ctx->N, nan);
        }
        cafe::GainDownHost down{out, {}, {}};
        return cafe::gain_dense_impl(ctx, who, params, lambdas, mus, nus, root_absent, n, family, lnl, &down);
    });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

int cafe_debug_gain_dense_posterior(cafe_ctx* ctx, double ms[8], double* flops) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    for (int k = 0; ms && k < 8; ++k) ms[k] = ctx->gain_dense_posterior_ms[k];
    if (flops) *flops = ctx->gain_dense_posterior_flops;
    return CAFE_OK;
}

int cafe_gain_leaf_predictive(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent,
                              int64_t n, const int64_t* family, const cafe_gain_leaf_predictive_out* out) {
    const char* const who = "cafe_gain_leaf_predictive";
    const int rc = cafe::guarded(ctx, who, [&] {
        if (!out) { cafe::set_err(ctx, "%s: out is required", who); return (int)CAFE_ERR_ARGUMENT; }
        std::vector<double> own_lnl;
        double* lnl = out->lnl;
        if (!lnl && n > 0) { own_lnl.resize((size_t)n); lnl = own_lnl.data(); }
        for (double* p : {out->mean, out->sd, out->p_below, out->p_obs, out->p_above})      // what no finite lnl replaces
            if (p && n > 0) std::fill(p, p + (size_t)n * ctx->n_taxa, std::numeric_limits<double>::quiet_NaN());
        cafe::GainPredictHost pred{out, {}};
        return cafe::gain_dense_impl(ctx, who, params, lambdas, mus, nus, root_absent, n, family, lnl, nullptr, &pred);
    });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

int cafe_debug_gain_predictive(cafe_ctx* ctx, double ms[7], double* flops) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    for (int k = 0; ms && k < 7; ++k) ms[k] = ctx->gain_predictive_ms[k];
    if (flops) *flops = ctx->gain_predictive_flops;
    return CAFE_OK;
}

int cafe_gain_marginal_dense(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent,
                             double level, int64_t n, const int64_t* family, const cafe_gain_marginal_out* out) {
    const char* const who = "cafe_gain_marginal_dense";
    const int rc = cafe::guarded_observed(ctx, who, [&] {       // the leaf summary has no instantiation for a missing cell
        if (!out || (n > 0 && (!out->mean || !out->mode || !out->lo || !out->hi || !out->p_increase || !out->p_decrease || !out->p_same))) {
            cafe::set_err(ctx, "%s: out with mean, mode, lo, hi, p_increase, p_decrease and p_same is required", who);
            return (int)CAFE_ERR_ARGUMENT;
        }
        if (!(level > 0.0 && level < 1.0)) { cafe::set_err(ctx, "%s: level must lie in (0, 1)", who); return (int)CAFE_ERR_ARGUMENT; }
        std::vector<double> own_lnl;
        double* lnl = out->lnl;
        if (!lnl && n > 0) { own_lnl.resize((size_t)n); lnl = own_lnl.data(); }
        if (n > 0) {                                   // what no finite lnl replaces
            const size_t nodes = (size_t)n * ctx->n_nodes;
            for (double* p : {out->mean, out->p_increase, out->p_decrease, out->p_same}) std::fill(p, p + nodes, std::numeric_limits<double>::quiet_NaN());
            for (int32_t* p : {out->mode, out->lo, out->hi}) std::fill(p, p + nodes, -1);
        }
        cafe::GainMarginalHost marg{out, level, {}, {}};
        return cafe::gain_dense_impl(ctx, who, params, lambdas, mus, nus, root_absent, n, family, lnl, nullptr, nullptr, &marg);
    });
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

int cafe_debug_gain_marginal(cafe_ctx* ctx, double ms[9], double* flops) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    for (int k = 0; ms && k < 9; ++k) ms[k] = ctx->gain_marginal_ms[k];
    if (flops) *flops = ctx->gain_marginal_flops;
    return CAFE_OK;
}
