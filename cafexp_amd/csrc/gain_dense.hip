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
// the interior nodes and of the leaves ("down" below).  cafe_gain_leaf_predictive and cafe_gain_marginal_dense walk the same
// depths with other kernels behind the weights: the fused leaf kernel, the split GEMM and the summaries.  cafe_gain_score_gradient
// keeps the transposed GEMM and adds a second outside panel, a Toeplitz GEMM and the score kernels (gain_gradient_kernel.h).
//
// How the file hangs together.  Every MFMA kernel -- the up GEMM, the transposed GEMM, the fused predictive kernel, the split GEMM --
// runs the ONE tile loop gain_dense_tile, told at compile time how the matrix holds A and which side of the diagonal to keep.
// Every kernel of the down pass behind the weights reads the ONE op GainNodeOp.  On the host the four entries are four modes
// (GainMode) of gain_dense_run behind one shell, gain_dense_entry: the checks and what the host decides alone, then GainPlan
// (keys, levels, depths, panel indices and the op tables -- host data only), GainLayout (the batch width the context's budget
// allows and the workspace's offsets) and gain_dense_batches (the launches).  A mode's outputs leave through one GainSink, which
// describes them as planes, and its launches are timed into one GainProfile of the context (cafe_ctx.h).
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

// grid (column blocks of 256, row blocks of 16, nodes); a thread owns one column and 16 sizes.  The body of the plain product
// and weights kernels.  init(i0, n, f, v): the elements before the children are multiplied in.
template <class Init>
__device__ __forceinline__ void gain_dense_node(const GainProdArgs& a, int child0, int n_children, int rows, int64_t dst, Init init) {
    const int i0 = blockIdx.y * kGdProdRows;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 >= rows || f >= a.ncols) return;
    const int n = min(kGdProdRows, rows - i0);
    double v[kGdProdRows];
    int lifts[kGdProdRows];                            // (not read: the untracked product)
    init(i0, n, f, v);
    gain_dense_times_children(a, child0, n_children, i0, n, f, a.col[f], v, lifts);
    double* __restrict__ out = a.panels + dst + (int64_t)i0 * a.ld + f;
#pragma unroll
    for (int j = 0; j < kGdProdRows; ++j)
        if (j < n) out[(int64_t)j * a.ld] = v[j];
}

__global__ __launch_bounds__(256) void gain_dense_product_kernel(const GainProdArgs a) {
    const GainProdOp op = a.ops[blockIdx.z];
    gain_dense_node(a, op.child0, op.n_children, op.rows, op.dst, [](int, int, int64_t, double (&v)[kGdProdRows]) {
#pragma unroll
        for (int j = 0; j < kGdProdRows; ++j) v[j] = 1.0;
    });
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

// The tile of every MFMA kernel of this file: acc = A[r0 .. r0 + 63][kb .. ke) X[kb .. ke)[c0 .. c0 + 127] over the K tiles [kb, ke)
// (kb a multiple of 16; the contraction itself is 0..nk-1 and every load is guarded by it and by nr).  acc is zeroed here and the
// function ends behind a barrier: the buffers are free for the caller's next tile.  With an empty range acc is zero.
//   AForm  how `mat` holds A.  kGdAColumn: A[r][k] = mat[k * ldp + r], the 64 consecutive sizes of a k are one load of a wave and
//          one LDS row -- the up GEMM.  kGdAStored: A[r][k] = mat[r * ldp + k], the matrix AS STORED with the contraction index
//          contiguous -- the down pass; its staging is described at the transposed GEMM below.
//   Side   0: the whole range.  +1 keeps k < r, -1 keeps k > r (kGdAStored only), inside the straddling tiles r0 <= k0 < r0 + 64
//          only -- every other tile of the range lies wholly on the kept side and is staged as it is.  The comparison is made
//          once, on the staging registers, as the tile is loaded, never in the MFMA loop.
//          kGdAToeplitz: A[r][k] = mat[k - r] for k > r, else 0 -- a strictly upper triangular Toeplitz matrix that is never
//          stored: `mat` is its one generating row and the tile is made on the staging registers, in the stored form's
//          arrangement (gain_gradient_kernel.h).
//   Shift  the right-hand side is X'[k] = (k + 1) X[k + 1] in place of X[k]; nk counts the rows of X' (one fewer than X has).
enum { kGdAColumn = 0, kGdAStored = 1, kGdAToeplitz = 2 };
typedef double gd4 __attribute__((ext_vector_type(4)));
template <int AForm, int Side, bool Shift = false>
__device__ __forceinline__ void gain_dense_tile(double (*As)[kGdKT * kGdLdA], double (*Xs)[kGdKT * kGdLdX], const double* __restrict__ mat,
                                                const double* __restrict__ X, int r0, int nr, int kb, int ke, int nk, int ldp, int64_t ld, int64_t c0,
                                                gd4 (&acc)[4][2]) {
    static_assert(Side == 0 || AForm == kGdAStored, "the diagonal mask is the stored form's");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int arow = tid >> 2, aq = tid & 3;           // kGdAStored: row of the tile, quad of k
    const int c = r0 + arow;                           // its row's size
    const double* __restrict__ Pt = AForm == kGdAStored ? mat + (int64_t)c * ldp : mat;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (gd4){0.0, 0.0, 0.0, 0.0};
    if (kb >= ke) return;                              // (block-uniform)
    double ra[4];
    double2 rx[4];
    auto load = [&](int k0) {
        if constexpr (AForm == kGdAColumn) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + lane, k = k0 + wave + 4 * u;
                ra[u] = (r < nr && k < nk) ? Pt[(int64_t)k * ldp + r] : 0.0;
            }
        } else if constexpr (AForm == kGdAToeplitz) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 4 * aq + u;
                ra[u] = (c < nr && k > c && k < nk) ? Pt[k - c] : 0.0;
            }
        } else {
            const bool straddle = Side != 0 && k0 >= r0 && k0 < r0 + kGdMT; // (block-uniform)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = k0 + 4 * aq + 2 * h;                          // (even: k < nk <= ldp keeps k + 1 inside the row)
                double2 v = make_double2(0.0, 0.0);
                if (c < nr && k < nk) {
                    v = *reinterpret_cast<const double2*>(Pt + k);
                    if (k + 1 >= nk) v.y = 0.0;
                    if (straddle) {                                         // the split
                        if (Side > 0 ? !(k < c) : !(k > c)) v.x = 0.0;
                        if (Side > 0 ? !(k + 1 < c) : !(k + 1 > c)) v.y = 0.0;
                    }
                }
                ra[2 * h] = v.x;
                ra[2 * h + 1] = v.y;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + wave + 4 * u;
            rx[u] = k < nk ? *reinterpret_cast<const double2*>(X + (int64_t)(k + (Shift ? 1 : 0)) * ld + c0 + 2 * lane) : make_double2(0.0, 0.0);
            if constexpr (Shift) { rx[u].x *= (double)(k + 1); rx[u].y *= (double)(k + 1); }
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if constexpr (AForm == kGdAColumn) As[buf][(wave + 4 * u) * kGdLdA + lane] = ra[u];
            else As[buf][(4 * aq + u) * kGdLdA + (arow ^ (aq << 3))] = ra[u];
            *reinterpret_cast<double2*>(&Xs[buf][(wave + 4 * u) * kGdLdX + 2 * lane]) = rx[u];
        }
    };
    load(kb);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += kGdKT, buf ^= 1) {
        const bool more = k0 + kGdKT < ke;
        if (more) load(k0 + kGdKT);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            double af[4], bf[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = As[buf][(4 * s4 + l4) * kGdLdA + ((16 * i + l15) ^ (AForm != kGdAColumn ? s4 << 3 : 0))];
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

// acc[i][j][q] is row r0 + 16 i + (lane >> 4) + 4 q, column c0 + 32 wave + 16 j + (lane & 15): the rows below nr go to `out`
__device__ __forceinline__ void gain_dense_tile_store(double* __restrict__ out, int r0, int nr, int64_t ld, int64_t c0, const gd4 (&acc)[4][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 16 * i + l4 + 4 * q;
                if (r < nr) out[(int64_t)r * ld + c0 + 32 * wave + 16 * j + l15] = acc[i][j][q];
            }
}

// grid (column tiles, row tiles of the tallest op, interior non-root nodes of the level)
__global__ __launch_bounds__(256) void gain_dense_gemm_kernel(const GainGemmArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][kGdKT * kGdLdA];
    __shared__ __attribute__((aligned(16))) double Xs[2][kGdKT * kGdLdX];
    const GainGemmOp op = a.ops[blockIdx.z];
    const int r0 = blockIdx.y * kGdMT;
    if (r0 >= op.nr) return;                           // (block-uniform, ahead of every barrier)
    const int64_t c0 = (int64_t)blockIdx.x * kGdCols;
    gd4 acc[4][2];
    gain_dense_tile<kGdAColumn, 0>(As, Xs, a.mats + op.Pt, a.panels + op.B, r0, op.nr, 0, a.nk, a.nk, a.ldp, a.ld, c0, acc);
    gain_dense_tile_store(a.panels + op.F, r0, op.nr, a.ld, c0, acc);
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
    gain_dense_node(a.p, op.child0, op.n_children, op.rows, op.dst, [&](int i0, int n, int64_t f, double (&v)[kGdProdRows]) {
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
    });
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
//
// GainNodeOp is the ONE op of the down pass behind the weights: per depth a table of the interior nodes (the root alone at depth
// 0, which no GEMM reads) and one of the leaves.  The transposed GEMM, the split GEMM and the interior outputs and summaries read
// the first, the leaf outputs and summaries and the fused predictive kernel the second.
struct GainNodeOp {
    int64_t outside, B, W, Pt;       // interior: outside (-1: the root, `mass`), B, w (-1 at the root) panels, the matrix; leaf: W, Pt
    int32_t node;
    int32_t n;                       // interior: the node's sizes 0..n-1 (R + 1 at the root, M + 1 below)
    int32_t rows;                    // rows(u): the parent's sizes, the contraction of the node's GEMM
    int32_t taxon;                   // leaf: its row of `counts`
};
struct GainGemmTArgs {
    const GainNodeOp* ops;
    const double* mats;
    double* panels;
    int64_t ld;
    int32_t nr, ldp;                 // rows c = 0..nr-1 of the outside panel
};

// grid (column tiles, row tiles of M + 1, interior non-root nodes of the depth)
__global__ __launch_bounds__(256) void gain_posterior_dense_gemm_t_kernel(const GainGemmTArgs a) {
    __shared__ __attribute__((aligned(16))) double As[2][kGdKT * kGdLdA];
    __shared__ __attribute__((aligned(16))) double Xs[2][kGdKT * kGdLdX];
    const GainNodeOp op = a.ops[blockIdx.z];
    const int r0 = blockIdx.y * kGdMT;
    const int64_t c0 = (int64_t)blockIdx.x * kGdCols;
    gd4 acc[4][2];
    gain_dense_tile<kGdAStored, 0>(As, Xs, a.mats + op.Pt, a.panels + op.W, r0, a.nr, 0, op.rows, op.rows, a.ldp, a.ld, c0, acc);
    gain_dense_tile_store(a.panels + op.outside, r0, a.nr, a.ld, c0, acc);
}

// ------------------------------------------------------------------------------------------------------- down: outputs
// Both output kernels: 64 columns per block, lanes along f, the sizes dealt to four waves and folded in a fixed order.
// res is [4][n_nodes][ld]: p_absent, mean, p_gain, p_loss; posterior, when asked for, [n_nodes][N][ld].  Everything / Z.
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
struct GainPredArgs {
    const GainNodeOp* ops;           // the depth's leaves: Pt, W, rows (the contraction) and taxon, the leaf's row of `counts` and of res
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
    const GainNodeOp op = a.ops[blockIdx.y];
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
        gain_dense_tile<kGdAStored, 0>(As, Xs, a.mats + op.Pt, a.panels + op.W, r0, nr, 0, op.rows, op.rows, a.ldp, ld, c0, acc);
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

// ----------------------------------------------------------------------------- down: score vectors in alpha, beta, r
#include "gain_gradient_kernel.h"

// ---------------------------------------------------------------------------------------------------------------- host
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

// A plain kernel or, in the scaled mode, its twin, which takes the plain kernel's argument and then its own
template <class A, class... X>
void launch_either(bool scaled, void (*plain)(A), dim3 plain_grid, void (*twin)(A, X...), dim3 twin_grid, hipStream_t s, const A& a, X... x) {
    if (scaled) hipLaunchKernelGGL(twin, twin_grid, dim3(256), 0, s, a, x...);
    else hipLaunchKernelGGL(plain, plain_grid, dim3(256), 0, s, a);
}
// CAFE_LAUNCH around it, its failure text included; args: launch_either's, in parentheses
#define GAIN_LAUNCH_EITHER(c, args)              \
    do {                                         \
        (void)hipGetLastError();                 \
        launch_either args;                      \
        HIP_TRY(c, hipGetLastError());           \
    } while (0)

// What the four entries are asked in common
struct GainCall {
    const cafe_params* pr;
    const double *lam, *mus, *nus;
    double root_absent;
    int64_t n;
    const int64_t* family;
    double level = 0.0;                                // the marginal entry's interval
};

// Where a call's answers go.  The mode says which down pass runs (kGainScore: none); the planes say what it leaves: every
// output but lnl is a plane [n][rows] of the caller's, rows = n_nodes or, in the predictive mode, n_taxa, in the order in which
// the mode's kernels write them ([planes][rows][ld] on the device).  A batch comes back by one 2-D copy per kind of plane into
// the staging below and is scattered from there.
struct GainSink {
    GainMode mode = kGainScore;
    double* lnl = nullptr;                             // [n]
    std::vector<double*> dst;                          // a null plane is computed and not delivered (the predictive entry)
    std::vector<int32_t*> idst;
    int rows = 0;
    double* posterior = nullptr;                       // optional block [n][rows][N] (the posterior entry)
    std::vector<double> res, post;                     // [planes][rows][nb], [rows][N][nb]
    std::vector<int32_t> ires;

    void resize(int64_t entries, int N) {
        res.resize(dst.size() * (size_t)rows * entries);
        ires.resize(idst.size() * (size_t)rows * entries);
        if (posterior) post.resize((size_t)rows * N * entries);
    }
    hipError_t copy_back(const double* d_res, const int32_t* d_ires, const double* d_post, int64_t ld, int64_t nb, int N, hipStream_t s) {
        hipError_t e = hipSuccess;                     // [..][ld] on the device, [..][nb] on the host
        if (!dst.empty())
            e = hipMemcpy2DAsync(res.data(), sizeof(double) * nb, d_res, sizeof(double) * ld, sizeof(double) * nb, dst.size() * (size_t)rows, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && !idst.empty())
            e = hipMemcpy2DAsync(ires.data(), sizeof(int32_t) * nb, d_ires, sizeof(int32_t) * ld, sizeof(int32_t) * nb, idst.size() * (size_t)rows, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && posterior)
            e = hipMemcpy2DAsync(post.data(), sizeof(double) * nb, d_post, sizeof(double) * ld, sizeof(double) * nb, (size_t)rows * N, hipMemcpyDeviceToHost, s);
        return e;
    }
    // lnl: the batch's.  An entry whose lnl is not finite keeps what its caller filled in: NaN, and -1 in the integers.
    void collect(int64_t b0, int64_t nb, int N, const double* lnl) const {
        const int nr = rows;                           // (locals: the scatter is the hot loop of a call on a short tree)
        for (int64_t b = 0; b < nb; ++b) {
            if (!std::isfinite(lnl[b])) continue;
            for (size_t k = 0; k < dst.size(); ++k) {
                double* const to = dst[k];
                if (!to) continue;
                const double* const from = res.data() + k * nr * nb + b;
                for (int v = 0; v < nr; ++v) to[(b0 + b) * nr + v] = from[(size_t)v * nb];
            }
            for (size_t k = 0; k < idst.size(); ++k) {
                int32_t* const to = idst[k];
                const int32_t* const from = ires.data() + k * nr * nb + b;
                for (int v = 0; v < nr; ++v) to[(b0 + b) * nr + v] = from[(size_t)v * nb];
            }
            if (!posterior) continue;
            double* po = posterior + (b0 + b) * nr * N;
            for (int64_t i = 0; i < (int64_t)nr * N; ++i) po[i] = post[(size_t)i * nb + b];
        }
    }
};

// ---- the checks every mode makes of its arguments and of the context
int gain_dense_check(cafe_ctx* c, const char* who, const GainCall& q, const double* family_lnl) {
    const cafe_params* pr = q.pr;
    if (!pr || !pr->prior) { set_err(c, "%s: params with a prior are required", who); return CAFE_ERR_ARGUMENT; }
    if (pr->model != CAFE_MODEL_BASE) { set_err(c, "%s: base model only", who); return CAFE_ERR_ARGUMENT; }
    if (c->comm) { set_err(c, "%s: not valid on a context with a communicator attached", who); return CAFE_ERR_STATE; }
    if (q.n < 0 || !q.lam || (q.n > 0 && (!q.family || !family_lnl))) { set_err(c, "%s: lambdas, family and family_lnl are required", who); return CAFE_ERR_ARGUMENT; }
    if ((c->n_dev > 0) != (pr->error_model != nullptr)) {
        set_err(c, "%s: error model %s but the problem was created with n_deviations=%d", who, pr->error_model ? "given" : "missing", c->n_dev);
        return CAFE_ERR_ARGUMENT;
    }
    if (!c->device_ready || !c->d_counts) { set_err(c, "%s: the context holds no family table", who); return CAFE_ERR_STATE; }
    for (int64_t i = 0; i < q.n; ++i)
        if (q.family[i] < -1 || q.family[i] >= c->F_all) {
            set_err(c, "%s: family index %lld outside -1..%lld", who, (long long)q.family[i], (long long)c->F_all - 1);
            return CAFE_ERR_ARGUMENT;
        }
    return gain_rates_check(c, who, 1, q.nus, q.root_absent);
}

// ---- what the host decides alone: an invalid rate set is -inf in every entry, a NaN lambda that passes the rule NaN
bool gain_dense_host_answer(cafe_ctx* c, const GainCall& q, double* family_lnl) {
    bool nan = false;
    for (int k = 0; k < c->n_lambdas; ++k) nan = nan || std::isnan(q.lam[k]);
    const bool valid = lambdas_valid(c, q.lam) && death_rates_ok(c->n_lambdas, q.mus);
    if (valid && !nan) return false;
    std::fill(family_lnl, family_lnl + q.n, valid ? std::numeric_limits<double>::quiet_NaN() : -std::numeric_limits<double>::infinity());
    return true;
}

// ---- the plan: everything a call fixes from the tree, the rates and the mode before the device is asked anything.  index()
// numbers the matrices and panels, which sizes the workspace; tables() then writes the op tables for the panel stride that the
// workspace allows.
struct GainPlan {
    // keys: one matrix per distinct (lambda index, quantized t)
    std::vector<SlotParamGain> slots;
    std::vector<int> node_key;
    // the up pass.  A node's height: 0 when its children are leaves, else 1 + its tallest interior child's; a level's product
    // reads the F panels of the levels below it, its GEMMs read the level's own B panels
    std::vector<int> height, bidx, fidx;
    int n_pan = 0, n_levels = 0;
    // the down pass (with `walk`): the nodes by depth (breadth first: parents in front of their children), an outside panel per
    // interior non-root node behind the up pass's panels, the w panels of the widest depth behind those
    std::vector<int> by_depth, depth_off{0}, oidx, widx;
    int n_down = 0, n_depths = 0;
    // the tables: per level its products and GEMMs and the tallest of each; per depth the weights of every node, the interior
    // nodes (at depth 0 the root alone) and the leaves
    std::vector<GainChild> children;
    std::vector<GainProdOp> prod_ops;
    std::vector<GainGemmOp> gemm_ops;
    std::vector<GainWeightOp> weight_ops;
    std::vector<GainNodeOp> int_ops, leaf_ops;
    std::vector<int> prod_off{0}, gemm_off{0}, prod_rows, gemm_rows, weight_off{0}, int_off{0}, leaf_off{0}, weight_rows;
    std::vector<double> reals;                         // log mass of the root sizes, then the error model
    std::vector<double> mass;                          // the root's outside vector (with `walk`)
    // the gradient mode: the keys that leaves have (three derivative matrices each), a key's place among them, the table
    // L[j] = beta^j / j of every key in rows of ldl doubles, and the first of the second outside panels (one per node of the widest depth)
    std::vector<int32_t> leaf_keys, dmat_of;
    std::vector<double> ltab;
    int ldl = 0, o2idx = 0;

    int n_keys() const { return (int)slots.size(); }

    int index(cafe_ctx* c, const char* who, const GainCall& q, bool walk, bool grad = false) {
        const int nn = c->n_nodes;
        std::map<std::pair<int, long>, int> key_of;
        node_key.assign(nn, -1); height.assign(nn, -1); bidx.assign(nn, -1); fidx.assign(nn, -1);
        for (int u = 0; u < nn; ++u) {
            if (u != c->root) {
                const auto it = key_of.emplace(std::make_pair(c->lam_idx[u], quantize_time(c->blen[u])), (int)slots.size());
                if (it.second) slots.push_back(gain_branch_slot(c, u, q.lam, q.mus, q.nus));
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
        oidx.assign(nn, -1); widx.assign(nn, -1);
        by_depth.assign(1, c->root);
        if (!walk) return CAFE_OK;
        std::vector<int> depth(nn, 0);
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
        if (!grad) return CAFE_OK;
        o2idx = n_pan + n_down;
        n_down += widest;
        dmat_of.assign(slots.size(), -1);
        for (int u = 0; u < nn; ++u)
            if (u != c->root && c->leaf_taxon[u] >= 0 && dmat_of[node_key[u]] < 0) {
                dmat_of[node_key[u]] = (int32_t)leaf_keys.size();
                leaf_keys.push_back(node_key[u]);
            }
        ldl = round_up(c->N, 16) + 16;
        ltab.assign(slots.size() * (size_t)ldl, 0.0);
        for (size_t k = 0; k < slots.size(); ++k) {
            double bj = 1.0;
            for (int j = 1; j <= c->M; ++j) {
                bj *= slots[k].beta;
                ltab[k * ldl + j] = bj / j;
            }
        }
        return CAFE_OK;
    }

    void tables(const cafe_ctx* c, const GainCall& q, bool walk, int64_t mat_stride, int64_t pan_stride) {
        const int nn = c->n_nodes, M = c->M, R = c->R;
        auto factor = [&](int v) {                     // the factor of node v in a product over its parent's sizes
            const bool leaf = c->leaf_taxon[v] >= 0;
            return GainChild{leaf ? node_key[v] * mat_stride : fidx[v] * pan_stride, leaf ? c->leaf_taxon[v] : -1, 0};
        };
        for (int lv = 0; lv < n_levels; ++lv) {
            int pr_rows = 0, gm_rows = 0;
            for (int u = 0; u < nn; ++u) {
                if (height[u] != lv) continue;
                GainProdOp po{};
                po.dst = bidx[u] * pan_stride;
                po.rows = (u == c->root ? R : M) + 1;
                po.child0 = (int32_t)children.size();
                for (int ch : c->children[u]) children.push_back(factor(ch));
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
                for (int sib : c->children[p])
                    if (sib != u) children.push_back(factor(sib));
                wo.n_children = (int32_t)children.size() - wo.child0;
                weight_ops.push_back(wo);
                w_rows = std::max(w_rows, rows);
                if (c->leaf_taxon[u] >= 0)
                    leaf_ops.push_back({-1, -1, widx[u] * pan_stride, node_key[u] * mat_stride, u, M + 1, rows, c->leaf_taxon[u]});
                else
                    int_ops.push_back({oidx[u] * pan_stride, bidx[u] * pan_stride, widx[u] * pan_stride, node_key[u] * mat_stride, u, M + 1, rows, -1});
            }
            weight_off.push_back((int)weight_ops.size());
            int_off.push_back((int)int_ops.size()); leaf_off.push_back((int)leaf_ops.size());
            weight_rows.push_back(w_rows);
        }
        reals.resize((size_t)R + 1 + (size_t)(M + 1) * c->n_dev);
        reals[0] = std::log(q.root_absent);
        for (int j = 0; j < R; ++j) reals[j + 1] = std::log1p(-q.root_absent) + std::log((double)q.pr->prior[j]);    // compute() returns float
        if (c->n_dev > 0) std::memcpy(reals.data() + R + 1, q.pr->error_model, sizeof(double) * (size_t)(M + 1) * c->n_dev);
        if (!walk) return;
        mass.resize((size_t)R + 1);
        mass[0] = q.root_absent;
        for (int j = 1; j <= R; ++j) mass[j] = (1.0 - q.root_absent) * (double)q.pr->prior[j - 1];
    }
};

// ---- the workspace: the tables in one blob at its front, then the batch's columns and lnl, the matrices (they stand once), the
// panels, and what the mode's down pass leaves.  Offsets are bytes from the workspace's base.  The columns, the matrices and the
// panels start on 4 KB: where they stand must not depend on the size of the tables in front of them -- at 256-byte steps the
// memory-bound kernels measured up to 5 % apart (leaf outputs, order 751) between two blob sizes 19 KB apart.  The 64 KB of
// slack in the budget's fixed part covers the three gaps.
constexpr size_t kGdRegion = 4096;
inline size_t gain_region_up(size_t v) { return (v + kGdRegion - 1) / kGdRegion * kGdRegion; }
struct GainLayout {
    int64_t entries = 0, ld = 0, mat_stride = 0, pan_stride = 0;   // entries per batch; columns of a panel; doubles per matrix and per panel
    int split_tiles = 0;                               // row tiles of the split GEMM: its partials are [n_nodes][tiles][3][ld]
    std::vector<char> blob;
    size_t o_children = 0, o_prod = 0, o_gemm = 0, o_slots = 0, o_reals = 0, o_weight = 0, o_int = 0, o_leaf = 0, o_mass = 0;
    size_t o_col = 0, o_out = 0, o_mats = 0, o_pan = 0, o_res = 0, o_post = 0, o_parts = 0, o_ires = 0, o_exps = 0, o_zt = 0, need = 0;
    size_t o_ltab = 0, o_leaf_keys = 0, o_dmat_of = 0, o_dmats = 0;    // the gradient mode's tables and derivative matrices

    void batch(const cafe_ctx* c, const GainCall& q, const GainSink& sink, bool scaled, const GainPlan& plan, size_t budget);
    void place(const cafe_ctx* c, const GainSink& sink, bool scaled, const GainPlan& plan);
};

// Columns per batch under `budget` bytes, from the plan's index alone: the matrices stand once, a batch adds its panels
void GainLayout::batch(const cafe_ctx* c, const GainCall& q, const GainSink& sink, bool scaled, const GainPlan& plan, size_t budget) {
    GainLayout& w = *this;
    const int nn = c->n_nodes, N = c->N, M = c->M, R = c->R, n_keys = plan.n_keys(), n_pan = plan.n_pan, n_down = plan.n_down;
    const bool walk = sink.mode != kGainScore, marg = sink.mode == kGainMarginal, grad = sink.mode == kGainGradient;
    const size_t planes = sink.dst.size() * (size_t)sink.rows, iplanes = sink.idst.size() * (size_t)sink.rows;
    w.mat_stride = (int64_t)N * round_up(N, 2);
    w.split_tiles = (M + kGdMT) / kGdMT;
    const size_t fixed_bytes = sizeof(double) * (size_t)w.mat_stride * n_keys + ((size_t)64 << 10) + sizeof(GainChild) * (size_t)nn +
                               sizeof(GainProdOp) * (size_t)nn + sizeof(GainGemmOp) * (size_t)nn + sizeof(SlotParamGain) * (size_t)n_keys +
                               sizeof(double) * ((size_t)R + 1 + (size_t)(M + 1) * c->n_dev) +
                               (walk ? (sizeof(GainChild) + sizeof(GainWeightOp) + sizeof(GainNodeOp)) * (size_t)nn + sizeof(double) * ((size_t)R + 1) : 0) +
                               (grad ? sizeof(double) * (3 * (size_t)w.mat_stride * plan.leaf_keys.size() + plan.ltab.size()) + 2 * sizeof(int32_t) * (size_t)n_keys + kGdRegion : 0);
    const size_t column_bytes = sizeof(double) * (size_t)n_pan * N + sizeof(int64_t) + sizeof(double) +
                                sizeof(double) * ((size_t)n_down * N + planes + (sink.posterior ? (size_t)nn * N : 0)) + sizeof(int32_t) * iplanes +
                                (marg ? sizeof(double) * 3 * (size_t)w.split_tiles * nn : 0) +                     // the split's partials
                                (grad ? sizeof(double) * (size_t)w.split_tiles * nn : 0) +                         // the Toeplitz GEMM's
                                (scaled ? sizeof(int32_t) * (size_t)(n_pan + n_down) + sizeof(double) : 0);     // the exponents, log Z~
    int64_t entries = budget > fixed_bytes ? (int64_t)((budget - fixed_bytes) / column_bytes) / kGdCols * kGdCols : 0;
    entries = std::max<int64_t>(kGdCols, std::min<int64_t>(entries, round_up64(q.n, kGdCols)));
    if (c->pf_max_batch > 0) entries = std::min(entries, c->pf_max_batch);
    w.entries = entries;
    w.ld = round_up64(entries, kGdCols);
    w.pan_stride = (int64_t)N * w.ld;
}

// The plan's tables in the blob and the offsets behind it
void GainLayout::place(const cafe_ctx* c, const GainSink& sink, bool scaled, const GainPlan& plan) {
    GainLayout& w = *this;
    const int nn = c->n_nodes, N = c->N, n_keys = plan.n_keys(), n_pan = plan.n_pan, n_down = plan.n_down;
    const bool marg = sink.mode == kGainMarginal, grad = sink.mode == kGainGradient;
    const size_t planes = sink.dst.size() * (size_t)sink.rows, iplanes = sink.idst.size() * (size_t)sink.rows;
    const int64_t ld = w.ld;
    w.o_children = put(w.blob, plan.children); w.o_prod = put(w.blob, plan.prod_ops); w.o_gemm = put(w.blob, plan.gemm_ops);
    w.o_slots = put(w.blob, plan.slots); w.o_reals = put(w.blob, plan.reals); w.o_weight = put(w.blob, plan.weight_ops);
    w.o_int = put(w.blob, plan.int_ops); w.o_leaf = put(w.blob, plan.leaf_ops); w.o_mass = put(w.blob, plan.mass);
    w.o_ltab = put(w.blob, plan.ltab); w.o_leaf_keys = put(w.blob, plan.leaf_keys); w.o_dmat_of = put(w.blob, plan.dmat_of);
    w.o_col = gain_region_up(w.blob.size());
    w.o_out = w.o_col + family_align_up(sizeof(int64_t) * ld);
    w.o_mats = gain_region_up(w.o_out + sizeof(double) * ld);
    w.o_dmats = gain_region_up(w.o_mats + sizeof(double) * (size_t)w.mat_stride * n_keys);
    w.o_pan = gain_region_up(w.o_dmats + sizeof(double) * 3 * (size_t)w.mat_stride * plan.leaf_keys.size());
    w.o_res = w.o_pan + sizeof(double) * (size_t)w.pan_stride * (n_pan + n_down);
    w.o_post = w.o_res + sizeof(double) * planes * ld;
    w.o_parts = w.o_post + (sink.posterior ? sizeof(double) * (size_t)nn * N * ld : 0);
    w.o_ires = w.o_parts + sizeof(double) * (marg ? 3 : grad ? 1 : 0) * (size_t)w.split_tiles * nn * ld;
    w.o_exps = w.o_ires + (iplanes ? family_align_up(sizeof(int32_t) * iplanes * ld) : 0);
    w.o_zt = w.o_exps + (scaled ? family_align_up(sizeof(int32_t) * (size_t)(n_pan + n_down) * ld) : 0);
    w.need = w.o_zt + (scaled ? sizeof(double) * ld : 0);
}

// The context's workspace, kept between calls, grown to the layout's need
int gain_dense_workspace(cafe_ctx* c, const char* who, const GainLayout& w, int n_keys) {
    if (w.need <= c->pf_dev_bytes) return CAFE_OK;
    if (c->pf_dev) { HIP_TRY(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->pf_dev); c->pf_dev = nullptr; c->pf_dev_bytes = 0; }
    if (hipMalloc(&c->pf_dev, w.need) != hipSuccess) {
        (void)hipGetLastError();
        c->pf_dev = nullptr;
        set_err(c, "%s: cannot allocate a workspace of %zu bytes (%d matrices of order %d, %lld columns per batch)", who, w.need, n_keys, c->N, (long long)w.ld);
        return CAFE_ERR_MEMORY;
    }
    c->pf_dev_bytes = w.need;
    return CAFE_OK;
}

// ---- the launches, batch by batch: the up pass level by level and the root kernel, then -- kGainScore apart -- by depth the
// weights of every node, the transposed GEMM of the interior ones (the marginal mode: the SPLIT GEMM in its place) and what the
// mode wants of the depth: the output kernels of every node (posterior), their summary kernels (marginal), or the fused kernel of
// the leaves alone (predictive).  prof: the launches' ms by kind and the MFMA flops issued.
int gain_dense_batches(cafe_ctx* c, const GainCall& q, const GainPlan& plan, const GainLayout& w, bool scaled, GainSink& sink, GainProfile& prof) {
    const int nn = c->n_nodes, N = c->N, M = c->M, R = c->R, ldp = round_up(N, 2);
    const int64_t ld = w.ld, n = q.n;
    const GainMode mode = sink.mode;
    char* base = static_cast<char*>(c->pf_dev);
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(base, w.blob.data(), w.blob.size(), hipMemcpyHostToDevice, s));
    GainTimer timer;
    timer.on = c->profile != 0;

    double* mats = reinterpret_cast<double*>(base + w.o_mats);
    double* panels = reinterpret_cast<double*>(base + w.o_pan);
    const double* d_reals = reinterpret_cast<const double*>(base + w.o_reals);
    const GainNodeOp* int_ops = reinterpret_cast<const GainNodeOp*>(base + w.o_int);
    const GainNodeOp* leaf_ops = reinterpret_cast<const GainNodeOp*>(base + w.o_leaf);
    GainBuildArgs ba{reinterpret_cast<const SlotParamGain*>(base + w.o_slots), mats, N, ldp, w.mat_stride};
    timer.mark(kGdBuild, s);
    HIP_TRY(c, launch_build(ba, plan.n_keys(), s));
    timer.mark(kGdBuild, s);

    GainProdArgs pa{};
    pa.ops = reinterpret_cast<const GainProdOp*>(base + w.o_prod); pa.children = reinterpret_cast<const GainChild*>(base + w.o_children);
    pa.panels = panels; pa.mats = mats; pa.col = reinterpret_cast<const int64_t*>(base + w.o_col);
    pa.counts = c->d_counts; pa.counts_ld = c->Fp; pa.ld = ld;
    pa.err = c->n_dev > 0 ? d_reals + R + 1 : nullptr;
    pa.n_dev = c->n_dev; pa.M = M; pa.ldp = ldp;
    GainGemmArgs ga{reinterpret_cast<const GainGemmOp*>(base + w.o_gemm), mats, panels, ld, M + 1, ldp};
    GainRootArgs ra{panels + plan.bidx[c->root] * w.pan_stride, d_reals, reinterpret_cast<double*>(base + w.o_out), ld, R,
                    mode != kGainScore || c->root_rule == CAFE_ROOT_SUM ? 1 : 0};      // every down pass forces the sum rule
    GainWeightArgs wa{pa, reinterpret_cast<const GainWeightOp*>(base + w.o_weight), reinterpret_cast<const double*>(base + w.o_mass)};
    GainGemmTArgs ta{int_ops, mats, panels, ld, M + 1, ldp};
    GainOutArgs oa{};
    oa.mats = mats; oa.panels = panels; oa.mass = wa.mass; oa.lnl = ra.out;
    oa.res = reinterpret_cast<double*>(base + w.o_res); oa.posterior = sink.posterior ? reinterpret_cast<double*>(base + w.o_post) : nullptr;
    oa.col = pa.col; oa.counts = pa.counts; oa.err = pa.err; oa.counts_ld = pa.counts_ld; oa.ld = ld;
    oa.nn = nn; oa.N = N; oa.M = M; oa.ldp = ldp; oa.n_dev = c->n_dev; oa.any_missing = c->has_missing ? 1 : 0;
    oa.root_B = plan.bidx[c->root] * w.pan_stride;
    GainPredArgs qa{leaf_ops, mats, panels, oa.res, pa.col, pa.counts, pa.err, pa.counts_ld, ld, M + 1, ldp, c->n_dev, c->n_taxa};
    const GainScaleArgs sa{reinterpret_cast<int32_t*>(base + w.o_exps), N};
    const int32_t* exps = sa.exps;
    const int32_t* root_exps = exps + plan.bidx[c->root] * ld;
    double* zt = reinterpret_cast<double*>(base + w.o_zt);
    if (scaled) oa.lnl = zt;                           // the outputs divide by Z~ = exp(log Z~)
    GainSplitArgs xa{int_ops, mats, panels, reinterpret_cast<double*>(base + w.o_parts), ld, M + 1, ldp};
    GainSummaryArgs ya{oa, xa.parts, reinterpret_cast<int32_t*>(base + w.o_ires), q.level, w.split_tiles};
    GainGradArgs da{};
    da.slots = ba.slots; da.mats = mats; da.panels = panels; da.ltab = reinterpret_cast<const double*>(base + w.o_ltab); da.parts = xa.parts;
    da.dmats = reinterpret_cast<double*>(base + w.o_dmats); da.leaf_keys = reinterpret_cast<const int32_t*>(base + w.o_leaf_keys);
    da.dmat_of = reinterpret_cast<const int32_t*>(base + w.o_dmat_of); da.lnl = ra.out; da.res = oa.res;
    da.col = pa.col; da.counts = pa.counts; da.err = pa.err; da.counts_ld = pa.counts_ld; da.ld = ld;
    da.mat_stride = w.mat_stride; da.pan_stride = w.pan_stride; da.o2 = plan.o2idx * w.pan_stride;
    da.nn = nn; da.N = N; da.M = M; da.ldp = ldp; da.ldl = plan.ldl; da.n_dev = c->n_dev; da.tiles = w.split_tiles;
    if (mode == kGainGradient && !plan.leaf_keys.empty()) {      // the derivative matrices of the leaf keys stand once, like the matrices
        const unsigned nk = (unsigned)plan.leaf_keys.size(), sb = (unsigned)((N + 63) / 64);
        timer.mark(kGdFilter, s);
        CAFE_LAUNCH(c, gain_gradient_filter_kernel, dim3(sb, nk), dim3(64), 0, s, da);
        CAFE_LAUNCH(c, gain_gradient_lambda_kernel, dim3(sb, (unsigned)((M + kGgChunk) / kGgChunk), nk), dim3(64), 0, s, da);
        timer.mark(kGdFilter, s);
    }
    sink.resize(w.entries, N);

    const double k_rows = round_up(M + 1, kGdMT);      // the rows a down-pass MFMA kernel issues for a node
    double flops = 0.0;
    std::vector<int64_t> col((size_t)ld);
    std::vector<double> res((size_t)ld);
    for (int64_t b0 = 0; b0 < n; b0 += w.entries) {
        const int64_t nb = std::min(w.entries, n - b0), cols = round_up64(nb, kGdCols);
        for (int64_t b = 0; b < cols; ++b) col[b] = (b < nb && q.family[b0 + b] >= 0) ? c->ref_of[q.family[b0 + b]] : -1;    // (padding: the absent profile)
        HIP_TRY(c, hipMemcpyAsync(base + w.o_col, col.data(), sizeof(int64_t) * cols, hipMemcpyHostToDevice, s));
        const unsigned tiles = (unsigned)(cols / kGdCols), blocks64 = (unsigned)(cols / 64), blocks256 = (unsigned)((cols + 255) / 256);
        for (int lv = 0; lv < plan.n_levels; ++lv) {
            const int np = plan.prod_off[lv + 1] - plan.prod_off[lv], ng = plan.gemm_off[lv + 1] - plan.gemm_off[lv];
            GainProdArgs p = pa;
            p.ops += plan.prod_off[lv];
            p.ncols = cols;
            timer.mark(kGdProduct, s);
            GAIN_LAUNCH_EITHER(c, (scaled, gain_dense_product_kernel, dim3(blocks256, (unsigned)((plan.prod_rows[lv] + kGdProdRows - 1) / kGdProdRows), (unsigned)np),
                                     gain_scaled_product_kernel, dim3(blocks64, (unsigned)np), s, p, sa));
            timer.mark(kGdProduct, s);
            if (ng == 0) continue;
            GainGemmArgs g = ga;
            g.ops += plan.gemm_off[lv];
            timer.mark(kGdGemm, s);
            CAFE_LAUNCH(c, gain_dense_gemm_kernel, dim3(tiles, (unsigned)((plan.gemm_rows[lv] + kGdMT - 1) / kGdMT), (unsigned)ng), dim3(256), 0, s, g);
            timer.mark(kGdGemm, s);
            for (int k = plan.gemm_off[lv]; k < plan.gemm_off[lv + 1]; ++k)
                flops += 2.0 * round_up(plan.gemm_ops[k].nr, kGdMT) * (double)round_up(M + 1, kGdKT) * (double)cols;
        }
        timer.mark(kGdRoot, s);
        GAIN_LAUNCH_EITHER(c, (scaled, gain_dense_root_kernel, dim3(blocks64), gain_scaled_root_kernel, dim3(blocks64), s, ra, root_exps, zt));
        timer.mark(kGdRoot, s);
        HIP_TRY(c, hipMemcpyAsync(res.data(), base + w.o_out, sizeof(double) * nb, hipMemcpyDeviceToHost, s));
        for (int d = 0; d < plan.n_depths; ++d) {      // the down pass: every B and F panel of the batch is still in place
            const int nw = plan.weight_off[d + 1] - plan.weight_off[d], ni = plan.int_off[d + 1] - plan.int_off[d],
                      nl = plan.leaf_off[d + 1] - plan.leaf_off[d], nt = d > 0 ? ni : 0;      // (depth 0 is the root: outputs, no GEMM)
            const GainNodeOp* const h_int = plan.int_ops.data() + plan.int_off[d];
            const GainNodeOp* const h_leaf = plan.leaf_ops.data() + plan.leaf_off[d];
            if (nw > 0) {
                GainWeightArgs wt = wa;
                wt.ops += plan.weight_off[d];
                wt.p.ncols = cols;
                timer.mark(kGdWeights, s);
                GAIN_LAUNCH_EITHER(c, (scaled, gain_posterior_dense_weights_kernel,
                                         dim3(blocks256, (unsigned)((plan.weight_rows[d] + kGdProdRows - 1) / kGdProdRows), (unsigned)nw),
                                         gain_scaled_weights_kernel, dim3(blocks64, (unsigned)nw), s, wt, sa));
                timer.mark(kGdWeights, s);
            }
            if (nt > 0 && mode == kGainMarginal) {     // the split GEMM: the outside panels and the three sums of every branch
                GainSplitArgs x = xa;
                x.ops += plan.int_off[d];
                timer.mark(kGdGemmT, s);
                CAFE_LAUNCH(c, gain_marginal_dense_split_kernel, dim3(tiles, (unsigned)w.split_tiles, (unsigned)nt), dim3(256), 0, s, x);
                timer.mark(kGdGemmT, s);
                for (int k = 0; k < nt; ++k)
                    for (int r0 = 0; r0 <= M; r0 += kGdMT) {               // the K tiles both phases issue, the masked repeats among them
                        const int k_end = round_up(h_int[k].rows, kGdKT);
                        flops += 2.0 * kGdMT * (double)(gain_marginal_phase1_end(r0, h_int[k].rows) + std::max(0, k_end - r0)) * (double)cols;
                    }
            } else if (nt > 0) {
                GainGemmTArgs t = ta;
                t.ops += plan.int_off[d];
                timer.mark(kGdGemmT, s);
                CAFE_LAUNCH(c, gain_posterior_dense_gemm_t_kernel, dim3(tiles, (unsigned)((M + kGdMT) / kGdMT), (unsigned)nt), dim3(256), 0, s, t);
                timer.mark(kGdGemmT, s);
                for (int k = 0; k < nt; ++k) flops += 2.0 * k_rows * (double)round_up(h_int[k].rows, kGdKT) * (double)cols;
            }
            if (mode == kGainGradient) {               // the second outside panels and the Toeplitz sums, then the three scores of every branch
                GainGradArgs g = da;
                g.ncols = cols;
                g.ops = int_ops + plan.int_off[d];
                if (nt > 0) {
                    const dim3 grid(tiles, (unsigned)w.split_tiles, (unsigned)nt);
                    timer.mark(kGdOutside2, s);
                    CAFE_LAUNCH(c, gain_gradient_outside2_kernel, grid, dim3(256), 0, s, g);
                    timer.mark(kGdOutside2, s);
                    timer.mark(kGdToeplitz, s);
                    CAFE_LAUNCH(c, gain_gradient_toeplitz_kernel, grid, dim3(256), 0, s, g);
                    timer.mark(kGdToeplitz, s);
                    for (int k = 0; k < nt; ++k) {
                        flops += 2.0 * k_rows * (double)round_up(h_int[k].rows - 1, kGdKT) * (double)cols;
                        for (int r0 = 0; r0 <= M; r0 += kGdMT) flops += 2.0 * kGdMT * (double)(round_up(M + 1, kGdKT) - r0) * (double)cols;
                    }
                }
                if (ni > 0) {
                    timer.mark(kGdInterior, s);
                    CAFE_LAUNCH(c, gain_gradient_interior_kernel, dim3(blocks256, (unsigned)ni), dim3(256), 0, s, g);
                    timer.mark(kGdInterior, s);
                }
                if (nl > 0) {
                    g.ops = leaf_ops + plan.leaf_off[d];
                    timer.mark(kGdLeaf, s);
                    CAFE_LAUNCH(c, gain_gradient_leaf_kernel, dim3(blocks64, (unsigned)nl), dim3(256), 0, s, g);
                    timer.mark(kGdLeaf, s);
                }
                continue;
            }
            if (mode == kGainPredictive) {             // the leaves' six sums straight from the MFMA accumulators; no other output
                if (nl == 0) continue;
                GainPredArgs pq = qa;
                pq.ops += plan.leaf_off[d];
                timer.mark(kGdPredict, s);
                CAFE_LAUNCH(c, gain_predictive_dense_leaf_kernel, dim3(tiles, (unsigned)nl), dim3(256), 0, s, pq);
                timer.mark(kGdPredict, s);
                for (int k = 0; k < nl; ++k) flops += 2.0 * k_rows * (double)round_up(h_leaf[k].rows, kGdKT) * (double)cols;
                continue;
            }
            // the outputs of every node of the depth; the marginal mode's summaries store nothing of a posterior
            GainSummaryArgs y = ya;
            GainOutArgs& o = y.o;
            if (ni > 0) {
                o.ops = int_ops + plan.int_off[d];
                timer.mark(kGdInterior, s);
                if (mode == kGainMarginal)
                    GAIN_LAUNCH_EITHER(c, (scaled, gain_marginal_dense_interior_kernel, dim3(blocks64, (unsigned)ni), gain_marginal_scaled_interior_kernel,
                                             dim3(blocks64, (unsigned)ni), s, y, exps));
                else
                    GAIN_LAUNCH_EITHER(c, (scaled, gain_posterior_dense_interior_kernel, dim3(blocks64, (unsigned)ni), gain_scaled_interior_kernel,
                                             dim3(blocks64, (unsigned)ni), s, o, exps));
                timer.mark(kGdInterior, s);
            }
            if (nl > 0) {
                o.ops = leaf_ops + plan.leaf_off[d];
                timer.mark(kGdLeaf, s);
                if (mode == kGainMarginal)
                    GAIN_LAUNCH_EITHER(c, (scaled, gain_marginal_dense_leaf_kernel, dim3(blocks64, (unsigned)nl), gain_marginal_scaled_leaf_kernel,
                                             dim3(blocks64, (unsigned)nl), s, y, exps));
                else
                    GAIN_LAUNCH_EITHER(c, (scaled, gain_posterior_dense_leaf_kernel, dim3(blocks64, (unsigned)nl), gain_scaled_leaf_kernel,
                                             dim3(blocks64, (unsigned)nl), s, o, exps));
                timer.mark(kGdLeaf, s);
            }
        }
        HIP_TRY(c, sink.copy_back(oa.res, ya.ires, oa.posterior, ld, nb, N, s));
        HIP_TRY(c, hipStreamSynchronize(s));            // the host tables of this batch go out of use
        std::copy(res.begin(), res.begin() + nb, sink.lnl + b0);
        sink.collect(b0, nb, N, res.data());
    }
    timer.collect(prof.ms);
    prof.flops = flops;
    return CAFE_OK;
}

// All four entries behind their shells.  The mode's record is zeroed on entry, ahead of the host-decided answers, and written
// when the call has run to its end; the other modes' records are not touched.
int gain_dense_run(cafe_ctx* c, const char* who, const GainCall& q, GainSink& sink) {
    if (const int rc = gain_dense_check(c, who, q, sink.lnl)) return rc;
    if (q.n == 0) return CAFE_OK;
    const bool grad = sink.mode == kGainGradient;
    const bool scaled = c->gain_scaling != 0 && !grad; // cafe_set_gain_scaling: the scaled twins of every kernel but the build and the GEMMs; the gradient mode has none
    c->last.state = LastCall::kNone;                   // cafe_family_results is not meaningful after this call
    c->gain_profile[sink.mode] = GainProfile{};
    if (gain_dense_host_answer(c, q, sink.lnl)) return CAFE_OK;
    GainPlan plan;
    if (const int rc = plan.index(c, who, q, sink.mode != kGainScore, grad)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    size_t budget = 0;
    HIP_TRY(c, workspace_budget(c->workspace_limit, c->pf_dev_bytes, &budget));
    GainLayout layout;
    layout.batch(c, q, sink, scaled, plan, budget);
    plan.tables(c, q, sink.mode != kGainScore, layout.mat_stride, layout.pan_stride);
    layout.place(c, sink, scaled, plan);
    if (const int rc = gain_dense_workspace(c, who, layout, plan.n_keys())) return rc;
    GainProfile prof;
    if (const int rc = gain_dense_batches(c, q, plan, layout, scaled, sink, prof)) return rc;
    c->gain_profile[sink.mode] = prof;
    return CAFE_OK;
}

// The shell of the four entries.  prepare(sink): the entry's own argument check, the fill of its outputs with what no finite lnl
// replaces, and the sink's planes.  An entry whose lnl is one output among others may leave it out: a stand-in takes it.
template <class Prepare>
int gain_dense_entry(cafe_ctx* ctx, const char* who, GainMode mode, const GainCall& q, Prepare prepare) {
    auto body = [&] {
        GainSink sink;
        sink.mode = mode;
        if (const int rc = prepare(sink)) return rc;
        std::vector<double> own_lnl;
        if (!sink.lnl && q.n > 0 && mode != kGainScore) { own_lnl.resize((size_t)q.n); sink.lnl = own_lnl.data(); }
        return gain_dense_run(ctx, who, q, sink);
    };
    // the marginal mode's leaf summary has no instantiation for a missing cell
    const int rc = mode == kGainMarginal ? guarded_observed(ctx, who, body) : guarded(ctx, who, body);
    if (rc == CAFE_ERR_DEVICE && ctx->device_ready && ctx->stream) (void)hipStreamSynchronize(ctx->stream);     // what the failed call left in flight
    return rc;
}

// A mode's record as its debug entry publishes it: the first `kinds` kinds
int gain_profile_read(cafe_ctx* ctx, GainMode mode, int kinds, double* ms, double* flops) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    for (int k = 0; ms && k < kinds; ++k) ms[k] = ctx->gain_profile[mode].ms[k];
    if (flops) *flops = ctx->gain_profile[mode].flops;
    return CAFE_OK;
}

// The chain rule of cafe_gain_score_gradient, per node in node order: the branch scores in (alpha, beta, r) of an entry -- raw
// [3][n][n_nodes] -- to the scores in the rates at the quantized key.  mus == nullptr: one free rate along mu = lambda.  A
// saturated key adds exactly 0 (and its three raw scores are delivered as 0); a rate index whose quantized lambda is 0 has NaN.
void gain_gradient_chain(const cafe_ctx* c, const GainCall& q, const std::vector<double>& lnl, std::vector<double>& raw, const cafe_gain_gradient_out* out) {
    const int nn = c->n_nodes, nl = c->n_lambdas;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t plane = (size_t)q.n * nn;
    bool any = false;
    for (int64_t i = 0; i < q.n; ++i) any = any || std::isfinite(lnl[i]);
    struct Coef { double al, am, bl, bm, rl, rn; int kind; };   // kind 0: saturated, 1: live, 2: lambda_q = 0
    std::vector<Coef> coef(nn, Coef{0, 0, 0, 0, 0, 0, 0});
    std::vector<char> poisson(nl, 0);
    for (int u = 0; any && u < nn; ++u) {
        if (u == c->root) continue;
        const int k = c->lam_idx[u];
        if (gain_branch_slot(c, u, q.lam, q.mus, q.nus).zero) continue;
        const long lq = quantize_lambda(q.lam[k]), mq = q.mus ? quantize_lambda(q.mus[k]) : lq;
        if (lq == 0) { coef[u].kind = 2; continue; }
        const double l = double(lq) / 1000000000.0, m = double(mq) / 1000000000.0, nu = double(quantize_lambda(q.nus[k])) / 1000000000.0;
        double g[4];
        bd_rates_grad(l, m, double(quantize_time(c->blen[u])) / 1000.0, g);
        coef[u] = Coef{g[0], g[1], g[2], g[3], -nu / (l * l), 1.0 / l, 1};
    }
    for (int k = 0; any && k < nl; ++k) poisson[k] = poisson[k] || quantize_lambda(q.lam[k]) == 0;
    for (int64_t i = 0; i < q.n; ++i) {
        if (out->lnl) out->lnl[i] = lnl[i];
        const bool ok = std::isfinite(lnl[i]);
        double* const ra = raw.data() + i * nn, *const rb = ra + plane, *const rr = rb + plane;
        if (!ok) for (double* r : {ra, rb, rr}) std::fill(r, r + nn, nan);
        for (int k = 0; k < nl; ++k) {
            double dl = 0.0, dm = 0.0, dn = 0.0;
            for (int u = 0; ok && u < nn; ++u) {
                if (u == c->root || c->lam_idx[u] != k) continue;
                const Coef& e = coef[u];
                if (e.kind != 1) { ra[u] = rb[u] = rr[u] = e.kind == 0 ? 0.0 : nan; continue; }
                if (q.mus) {
                    dl += (ra[u] * e.al + rb[u] * e.bl) + rr[u] * e.rl;
                    dm += ra[u] * e.am + rb[u] * e.bm;
                } else {
                    dl += (ra[u] * (e.al + e.am) + rb[u] * (e.bl + e.bm)) + rr[u] * e.rl;
                }
                dn += rr[u] * e.rn;
            }
            const bool bad = !ok || poisson[k];
            if (out->d_lambda) out->d_lambda[i * nl + k] = bad ? nan : dl;
            if (out->d_mu && q.mus) out->d_mu[i * nl + k] = bad ? nan : dm;
            if (out->d_nu) out->d_nu[i * nl + k] = bad ? nan : dn;
        }
        double* const to[3] = {out->d_alpha, out->d_beta, out->d_r};
        const double* const from[3] = {ra, rb, rr};
        for (int p = 0; p < 3; ++p)
            if (to[p]) std::copy(from[p], from[p] + nn, to[p] + i * nn);
    }
}

}  // namespace
}  // namespace cafe

int cafe_gain_score_gradient(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent,
                             int64_t n, const int64_t* family, const cafe_gain_gradient_out* out) {
    const char* const who = "cafe_gain_score_gradient";
    const cafe::GainCall q{params, lambdas, mus, nus, root_absent, n, family};
    std::vector<double> raw, lnl;
    const int rc = cafe::gain_dense_entry(ctx, who, cafe::kGainGradient, q, [&](cafe::GainSink& sink) {
        if (!out) { cafe::set_err(ctx, "%s: out is required", who); return (int)CAFE_ERR_ARGUMENT; }
        const size_t entries = n > 0 ? (size_t)n : 0, plane = entries * ctx->n_nodes;
        raw.assign(3 * plane, std::numeric_limits<double>::quiet_NaN());
        lnl.assign(entries, std::numeric_limits<double>::quiet_NaN());
        sink.lnl = lnl.data();
        sink.dst = {raw.data(), raw.data() + plane, raw.data() + 2 * plane};
        sink.rows = ctx->n_nodes;
        return (int)CAFE_OK;
    });
    if (rc != CAFE_OK || n <= 0) return rc;
    return cafe::guarded(ctx, who, [&] { cafe::gain_gradient_chain(ctx, q, lnl, raw, out); return (int)CAFE_OK; });
}

// the posterior entry's eight (interior and leaf: the score kernels), the second outside GEMM, the Toeplitz GEMM, the leaf filters;
// then their total
int cafe_debug_gain_gradient(cafe_ctx* ctx, double ms[12], double* flops) {
    const int rc = cafe::gain_profile_read(ctx, cafe::kGainGradient, 8, ms, flops);
    if (rc != CAFE_OK || !ms) return rc;
    ms[8] = ctx->gain_profile[cafe::kGainGradient].ms[cafe::kGdOutside2];
    ms[9] = ctx->gain_profile[cafe::kGainGradient].ms[cafe::kGdToeplitz];
    ms[10] = ctx->gain_profile[cafe::kGainGradient].ms[cafe::kGdFilter];
    ms[11] = 0.0;
    for (int k = 0; k < 11; ++k) ms[11] += ms[k];
    return rc;
}

int cafe_score_gain(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent, int64_t n,
                    const int64_t* family, double* family_lnl) {
    return cafe::gain_dense_entry(ctx, "cafe_score_gain", cafe::kGainScore, {params, lambdas, mus, nus, root_absent, n, family}, [&](cafe::GainSink& sink) {
        sink.lnl = family_lnl;
        return (int)CAFE_OK;
    });
}

int cafe_set_gain_scaling(cafe_ctx* ctx, int on) {
    if (!ctx) return CAFE_ERR_ARGUMENT;
    ctx->gain_scaling = on != 0;
    return CAFE_OK;
}

int cafe_debug_gain_dense(cafe_ctx* ctx, double ms[4], double* flops) { return cafe::gain_profile_read(ctx, cafe::kGainScore, 4, ms, flops); }

int cafe_gain_posterior_dense(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent,
                              int64_t n, const int64_t* family, const cafe_gain_posterior_out* out) {
    const char* const who = "cafe_gain_posterior_dense";
    return cafe::gain_dense_entry(ctx, who, cafe::kGainPosterior, {params, lambdas, mus, nus, root_absent, n, family}, [&](cafe::GainSink& sink) {
        if (!out || (n > 0 && (!out->p_absent || !out->mean || !out->p_gain || !out->p_loss))) {
            cafe::set_err(ctx, "%s: out with p_absent, mean, p_gain and p_loss is required", who);
            return (int)CAFE_ERR_ARGUMENT;
        }
        sink.lnl = out->lnl;
        sink.dst = {out->p_absent, out->mean, out->p_gain, out->p_loss};
        sink.rows = ctx->n_nodes;
        sink.posterior = out->posterior;
        if (n > 0) {
            const size_t nodes = (size_t)n * ctx->n_nodes;
            for (double* p : sink.dst) std::fill(p, p + nodes, std::numeric_limits<double>::quiet_NaN());
            if (out->posterior) std::fill(out->posterior, out->posterior + nodes * ctx->N, std::numeric_limits<double>::quiet_NaN());
        }
        return (int)CAFE_OK;
    });
}

int cafe_debug_gain_dense_posterior(cafe_ctx* ctx, double ms[8], double* flops) { return cafe::gain_profile_read(ctx, cafe::kGainPosterior, 8, ms, flops); }

int cafe_gain_leaf_predictive(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent,
                              int64_t n, const int64_t* family, const cafe_gain_leaf_predictive_out* out) {
    const char* const who = "cafe_gain_leaf_predictive";
    return cafe::gain_dense_entry(ctx, who, cafe::kGainPredictive, {params, lambdas, mus, nus, root_absent, n, family}, [&](cafe::GainSink& sink) {
        if (!out) { cafe::set_err(ctx, "%s: out is required", who); return (int)CAFE_ERR_ARGUMENT; }
        sink.lnl = out->lnl;
        sink.dst = {out->mean, out->sd, out->p_below, out->p_obs, out->p_above};
        sink.rows = ctx->n_taxa;
        for (double* p : sink.dst)
            if (p && n > 0) std::fill(p, p + (size_t)n * ctx->n_taxa, std::numeric_limits<double>::quiet_NaN());
        return (int)CAFE_OK;
    });
}

// build, product, GEMM, root, weights, transposed GEMM, and the fused leaf kernel in the seventh slot
int cafe_debug_gain_predictive(cafe_ctx* ctx, double ms[7], double* flops) {
    const int rc = cafe::gain_profile_read(ctx, cafe::kGainPredictive, 6, ms, flops);
    if (rc == CAFE_OK && ms) ms[6] = ctx->gain_profile[cafe::kGainPredictive].ms[cafe::kGdPredict];
    return rc;
}

int cafe_gain_marginal_dense(cafe_ctx* ctx, const cafe_params* params, const double* lambdas, const double* mus, const double* nus, double root_absent,
                             double level, int64_t n, const int64_t* family, const cafe_gain_marginal_out* out) {
    const char* const who = "cafe_gain_marginal_dense";
    return cafe::gain_dense_entry(ctx, who, cafe::kGainMarginal, {params, lambdas, mus, nus, root_absent, n, family, level}, [&](cafe::GainSink& sink) {
        if (!out || (n > 0 && (!out->mean || !out->mode || !out->lo || !out->hi || !out->p_increase || !out->p_decrease || !out->p_same))) {
            cafe::set_err(ctx, "%s: out with mean, mode, lo, hi, p_increase, p_decrease and p_same is required", who);
            return (int)CAFE_ERR_ARGUMENT;
        }
        if (!(level > 0.0 && level < 1.0)) { cafe::set_err(ctx, "%s: level must lie in (0, 1)", who); return (int)CAFE_ERR_ARGUMENT; }
        sink.lnl = out->lnl;
        sink.dst = {out->mean, out->p_increase, out->p_decrease, out->p_same};
        sink.idst = {out->mode, out->lo, out->hi};
        sink.rows = ctx->n_nodes;
        if (n > 0) {
            const size_t nodes = (size_t)n * ctx->n_nodes;
            for (double* p : sink.dst) std::fill(p, p + nodes, std::numeric_limits<double>::quiet_NaN());
            for (int32_t* p : sink.idst) std::fill(p, p + nodes, -1);
        }
        return (int)CAFE_OK;
    });
}

// the posterior entry's eight, the split GEMM sixth; then their total
int cafe_debug_gain_marginal(cafe_ctx* ctx, double ms[9], double* flops) {
    const int rc = cafe::gain_profile_read(ctx, cafe::kGainMarginal, 8, ms, flops);
    if (rc != CAFE_OK || !ms) return rc;
    ms[8] = 0.0;
    for (int k = 0; k < 8; ++k) ms[8] += ms[k];
    return rc;
}
