// Internal: the up pass of sum-products that cafe_marginal_reconstruct (marginal.hip) and cafe_sample_histories (history.hip)
// share -- F_v[i] = sum_j P_v[i][j] B_v[j], B_p[i] = prod_{children} F_c[i], the leaves gathered with the error model's taps.
// The kernels and both functions live in marginal.hip; a caller owns the two panel arenas.  cafe_score_gradient
// (gradient.hip) runs the same up pass and the same GEMM launches.  Host only.
#pragma once
#include <vector>

#include "cafe_call.h"

namespace cafe {

// B and F of every interior node: arena + bidx[v] * pstride is node v's panel, [size 0..N-1][column] with `pstride / N` columns
struct UpPanels {
    double* B = nullptr;
    double* F = nullptr;
    int64_t pstride = 0;
    std::vector<int> bidx;              // [n_nodes] index among the interior nodes, -1 for a leaf
    const double* err = nullptr;        // device copy of the call's error model, or nullptr
    int n_dev = 1;
    double* panel(double* arena, int v) const { return arena + (int64_t)bidx[v] * pstride; }
};

// HIP-event brackets of the GEMM launches (cafe_set_profiling): summed after the call
struct GemmTimer {
    bool on = false;
    std::vector<hipEvent_t> ev;
    double flops = 0.0;
    ~GemmTimer() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void mark(hipStream_t s) {
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
        ev.push_back(e);
        (void)hipEventRecord(e, s);
    }
    double total_ms() const {
        double t = 0.0;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) t += ms;
        }
        return t;
    }
};

// The fp64 MFMA GEMM of both passes (marginal_gemm_kernel, marginal.hip), one launch per branch
enum { kUp = 0, kDown = 1, kSplit = 2 };

struct GemmParams {
    const double* Pt;       // k-major matrix of the branch above v
    int ldp;
    const double* X;        // up: B_v (rows = sizes of v); down / split: G_v (rows = sizes of v's parent)
    int64_t ld;             // columns of every panel of the batch (a multiple of 128)
    int nr;                 // output rows: up: parent sizes 1..nr; down / split: sizes 0..nr-1 of v
    int nk;                 // contraction: up: sizes 0..nk-1 of v; down / split: parent sizes 1..nk
    int mask;               // split: 1 keeps i < j (the branch expanded), 2 keeps i > j (it contracted)
    double* out1;           // up: F_v;  down: O_v;  split: D
    double* out2;           // up: B_parent (store or multiply);  down: the node's accumulation panel
    const double* Bv;       // down / split: B_v
    double pk;              // down: weight of the category
    int first;              // down: first category (the accumulation panel is stored, not added to)
};

// One GEMM launch between the timer's marks; share: the part of its K tiles that runs.  Instantiated in marginal.hip for
// kUp (mul: multiply into out2 instead of storing), kDown and kSplit.
template <int MODE>
int launch_gemm(cafe_ctx* c, const GemmParams& g, bool mul, hipStream_t s, GemmTimer& timer, double share = 1.0);

// dst[i][f] = (src0 ? src0[i][f] : 1) * the factors of the nodes `mult` in category k (an interior node: its stored F panel,
// a leaf: gathered from its matrix), rows 0..nrows-1 of the columns f0 .. f0 + ld
int marginal_product(cafe_ctx* c, const UpPanels& w, const double* src0, double* dst, int nrows, const std::vector<int>& mult, int k, int64_t f0, int64_t ld,
                     hipStream_t s);
// The up pass of category k over the columns f0 .. f0 + ld, children before parents: afterwards B and F of every interior
// node hold that category's values (B_root over sizes 0..R, every other panel over 0..M)
int marginal_up_pass(cafe_ctx* c, const UpPanels& w, int k, int64_t f0, int64_t ld, hipStream_t s, GemmTimer& timer);

}  // namespace cafe
