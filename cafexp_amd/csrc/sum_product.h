// Internal: what cafe_marginal_reconstruct (marginal.hip), cafe_sample_histories (history.hip), cafe_score_gradient
// (gradient.hip), cafe_expected_events (events.hip) and cafe_leaf_predictive (predictive.hip) share.  The engine (sum_product.hip): the up pass of sum-products, F_v[i] = sum_j P_v[i][j] B_v[j], B_p[i] =
// prod_{children} F_c[i], the leaves gathered with the error model's taps, its fp64 MFMA GEMM and product kernel, the down pass's
// walk.  The frame, on top of cafe_call.h: argument checks, opening, constants, the test for a failed family, closing.
#pragma once
#include <cfloat>
#include <limits>
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
    // B and F at the head of a workspace; -> what follows them
    double* place(void* base, int nI, int64_t stride) { B = static_cast<double*>(base); F = B + nI * stride; pstride = stride; return F + nI * stride; }
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

// The fp64 MFMA GEMM of both passes (marginal_gemm_kernel), one launch per branch
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

// One GEMM launch between the timer's marks; share: the part of its K tiles that runs.  Instantiated for kUp (mul: multiply
// into out2 instead of storing), kDown and kSplit.
template <int MODE>
int launch_gemm(cafe_ctx* c, const GemmParams& g, bool mul, hipStream_t s, GemmTimer& timer, double share = 1.0);

// dst[i][f] = (src0 ? src0[i][f] : 1) * the factors of the nodes `mult` in category k (an interior node: its stored F panel,
// a leaf: gathered from its matrix), rows 0..nrows-1 of the columns f0 .. f0 + ld
int marginal_product(cafe_ctx* c, const UpPanels& w, const double* src0, double* dst, int nrows, const std::vector<int>& mult, int k, int64_t f0, int64_t ld,
                     hipStream_t s);
// The up pass of category k over the columns f0 .. f0 + ld, children before parents: afterwards B and F of every interior
// node hold that category's values (B_root over sizes 0..R, every other panel over 0..M)
int marginal_up_pass(cafe_ctx* c, const UpPanels& w, int k, int64_t f0, int64_t ld, hipStream_t s, GemmTimer& timer);

// The down pass's walk: the branch above every child v of every interior node p, parents before children; sizes 1..np of p
// index the rows of v's matrix, sib are v's siblings
struct Branch { int p, v, np; std::vector<int> sib; };
std::vector<Branch> branches_down(const cafe_ctx* c);
// One branch of that walk: G = O_p times the siblings' factors and, for an interior v, the kDown launch's parameters except
// out2 and first, which are the caller's (O: the arena of the O panels, G: one panel)
int down_branch(cafe_ctx* c, const UpPanels& w, double* O, double* G, const Branch& b, int k, double pk, int64_t f0, int64_t ld, hipStream_t s, GemmParams* g);

// The kernels of gradient.hip that cafe_expected_events (events.hip) launches too, one block of 256 threads per 256 columns:
// the root weight O_root and Z_k of a category (rule: CAFE_ROOT_MAX / CAFE_ROOT_SUM); acc[f] += pk sum_{i = 1..np} i G[i][f]
// Ft[i-1][f]; a leaf branch's acc0 / acc1[f] += pk sum_taps err sum_i G[i][f] dP0 / dP1[i][tap] (dP1, acc1 may be nullptr);
// Z = sum_k p_k Z_k, its logarithm (or lbest) and the n_acc sums of every column divided by it, NaN for a failed column
int launch_root_weights(cafe_ctx* c, hipStream_t s, const double* B, const double* prior, const double* logprior, int R, int64_t ld, double* O, double* zk,
                        double* lbest, int rule, int use_log);
int launch_weighted_dot(cafe_ctx* c, hipStream_t s, const double* G, const double* Ft, int np, int64_t ld, double pk, double* acc);
int launch_leaf_sums(cafe_ctx* c, hipStream_t s, const double* G, int np, int64_t ld, const double* dP0, const double* dP1, int ldp, const int32_t* cnt,
                     const double* err, int n_dev, int M, double pk, double* acc0, double* acc1);
int launch_finish_sums(cafe_ctx* c, hipStream_t s, const double* zk, const double* probs, int K, int64_t ld, int64_t stride, const double* lbest, double* acc,
                       int n_acc, double* Z, double* lnl);

// The score panel of cafe_branch_scores (branch_scores.hip): S [P][Fp], one row per entry of the score vector z, one column
// per distinct family, kept on the device over all column batches.  Rows: the log-rate scores of the non-root nodes in node
// order (births, then deaths, while death rates are set), then the n_glob global scores.  The walk adds into a branch's row
// as it adds into the sums per lambda index; per batch the rows are divided by Z (a failed column: zeros), the global scores
// come from the host, which has just formed them, and the per-family rows go out; after the last batch the Gram matrix.
struct ScorePanel {
    const cafe_branch_scores_out* out = nullptr;
    int n_par = 1, n_branch = 0, n_glob = 0, P = 0;
    int64_t Fp = 0;
    std::vector<int> slot;              // [n_nodes] index among the non-root nodes, -1 at the root
    std::vector<char> col_failed;       // [Fp]
    DevBuf S;
    double* base() const { return static_cast<double*>(S.p); }
};
int score_panel_open(cafe_ctx* c, const char* entry, int n_par, int n_glob, ScorePanel* sp);
inline double* score_panel_row(const ScorePanel* sp, int v, int p, int64_t f0) { return sp->base() + ((int64_t)p * sp->n_branch + sp->slot[v]) * sp->Fp + f0; }
int score_panel_batch(cafe_ctx* c, hipStream_t s, ScorePanel* sp, int64_t f0, int64_t ld, int64_t cols, const double* d_Z, const double* h_Z, const double* h_glob);
int score_panel_close(cafe_ctx* c, hipStream_t s, ScorePanel* sp);
// cafe_score_gradient's checks, passes and outputs under the error prefix `entry`; sp: nullptr, or the panel to fill
int gradient_walk(cafe_ctx* c, const char* entry, const cafe_params* pr, int32_t root_rule, const cafe_gradient_out* out, ScorePanel* sp);

// ------------------------------------------------------------------------------------- the frame of the posterior calls
// A family whose evidence Z is zero, negative, NaN or infinite has failed: its doubles are kNaN
__host__ __device__ inline bool evidence_failed(double z) { return !(z > 0.0) || z > DBL_MAX; }
constexpr double kNaN = std::numeric_limits<double>::quiet_NaN();

// The argument checks, `entry` the C ABI name that opens the error text: communicator and required pointers, then -- behind
// the call's own range checks -- gamma categories, rates and error model
inline int check_call_args(cafe_ctx* c, const char* entry, const cafe_params* pr, const void* out) {
    if (c->comm) { set_err(c, "%s: not valid on a context with a communicator attached", entry); return CAFE_ERR_STATE; }
    if (!pr || !pr->lambdas || !pr->prior || !out) { set_err(c, "%s: lambdas, prior and out are required", entry); return CAFE_ERR_ARGUMENT; }
    return CAFE_OK;
}
inline int check_model_args(cafe_ctx* c, const char* entry, const cafe_params* pr) {
    const int K = pr->n_categories;
    if (pr->model == CAFE_MODEL_GAMMA && (K < 1 || K > c->Kmax || !pr->multipliers || !pr->cat_probs)) {
        set_err(c, "%s: gamma model needs 1..%d categories with multipliers and cat_probs", entry, c->Kmax);
        return CAFE_ERR_ARGUMENT;
    }
    if (!rates_valid(c, pr->lambdas)) { set_err(c, "%s: invalid lambda or death rate", entry); return CAFE_ERR_ARGUMENT; }
    if (pr->error_model && c->n_dev < 1) { set_err(c, "%s: the context was created without an error model", entry); return CAFE_ERR_ARGUMENT; }
    return CAFE_OK;
}

// An open call: begin_matrix_call done, the interior nodes indexed (up.bidx, nI; the panel arenas of `up` are the caller's).
// The constants -- the prior as doubles, its logarithms when asked for, the category weights (1.0: base model), the error
// model (up.err) -- are one device buffer: alloc_constants stands in the caller's chain of allocations, where the buffers
// it replaces stood, so a failure is reported with the workspace's; upload_constants is one copy and one synchronise.
enum PriorLogs { kNoPriorLogs, kWithPriorLogs };
struct PosteriorCall {
    hipStream_t s = nullptr;
    bool gamma = false, has_err = false;
    int K = 1, n_dev = 1, nI = 0;       // categories; taps of the error model (1 without); interior nodes
    UpPanels up;
    GemmTimer timer;                    // off unless the caller turns it on
    DevBuf consts;
    size_t n_consts = 0;
    const double *prior = nullptr, *logprior = nullptr, *probs = nullptr;
};
int open_posterior_call(cafe_ctx* c, const cafe_params* pr, PosteriorCall* pc);
hipError_t alloc_constants(const cafe_ctx* c, PriorLogs logs, PosteriorCall* pc);
int upload_constants(cafe_ctx* c, const cafe_params* pr, PosteriorCall* pc);
// The call succeeded: its matrices stay readable, scorer results are not meaningful; a timer's totals go to cafe_debug_marginal_gemm
inline void close_posterior_call(cafe_ctx* c, const GemmTimer* timer) {
    c->upload_pending = false;
    c->last.state = LastCall::kMatricesOnly;
    if (!timer) return;
    c->marginal_gemm_ms = timer->on ? timer->total_ms() : 0.0;
    c->marginal_gemm_flops = timer->flops;
}

}  // namespace cafe
