// Internal: the up pass of sum-products that cafe_marginal_reconstruct (marginal.hip) and cafe_sample_histories (history.hip)
// share -- F_v[i] = sum_j P_v[i][j] B_v[j], B_p[i] = prod_{children} F_c[i], the leaves gathered with the error model's taps.
// The kernels and both functions live in marginal.hip; a caller owns the two panel arenas.  Host only.
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

// dst[i][f] = (src0 ? src0[i][f] : 1) * the factors of the nodes `mult` in category k (an interior node: its stored F panel,
// a leaf: gathered from its matrix), rows 0..nrows-1 of the columns f0 .. f0 + ld
int marginal_product(cafe_ctx* c, const UpPanels& w, const double* src0, double* dst, int nrows, const std::vector<int>& mult, int k, int64_t f0, int64_t ld,
                     hipStream_t s);
// The up pass of category k over the columns f0 .. f0 + ld, children before parents: afterwards B and F of every interior
// node hold that category's values (B_root over sizes 0..R, every other panel over 0..M)
int marginal_up_pass(cafe_ctx* c, const UpPanels& w, int k, int64_t f0, int64_t ld, hipStream_t s, GemmTimer& timer);

}  // namespace cafe
