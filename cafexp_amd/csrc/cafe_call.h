// Internal: the host frame of a call on a context -- what the entry points beside the scorer (reconstruct.hip, marginal.hip,
// pvalues.hip, family_lambda.hip) share instead of copying it from one another.  Host only, plain functions.
#pragma once
#include <exception>
#include <string>

#include "cafe_ctx.h"

namespace cafe {

// The shell of a C ABI entry: a null context is an argument error; an exception (a host allocation) leaves
// "<entry>: <what>" as the context's error and returns CAFE_ERR_MEMORY
template <class Fn>
int guarded(cafe_ctx* c, const char* entry, Fn&& fn) {
    if (!c) return CAFE_ERR_ARGUMENT;
    try { return fn(); }
    catch (const std::exception& e) { set_err(c, "%s: %s", entry, e.what()); return CAFE_ERR_MEMORY; }
}

// The shell of an entry whose kernels index by the observed count and have no instantiation for CAFE_COUNT_MISSING: a context
// whose table has missing cells is refused here, before the entry touches the device -- such a kernel must never see a -1.
// The context stays as it was.
template <class Fn>
int guarded_observed(cafe_ctx* c, const char* entry, Fn&& fn) {
    if (!c) return CAFE_ERR_ARGUMENT;
    if (c->has_missing) { set_err(c, "%s: the table has missing cells (CAFE_COUNT_MISSING); this call is not available for such a context", entry); return CAFE_ERR_STATE; }
    return guarded(c, entry, fn);
}

// One kernel launch of an *_impl: a stale error of the thread is cleared first, so that what is reported belongs to this launch
#define CAFE_LAUNCH(c, kernel, grid, block, shmem, stream, ...)                  \
    do {                                                                         \
        (void)hipGetLastError();                                                 \
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);     \
        HIP_TRY(c, hipGetLastError());                                           \
    } while (0)

// Every call that builds matrices opens here: nothing of the call before it is readable any more, and what this one leaves
// becomes readable when it sets its final state (LastCall, cafe_ctx.h)
inline void open_call(cafe_ctx* c, int K, hipStream_t s) {
    c->last.state = LastCall::kNone;
    c->last.stream = s;
    c->last.K = K;
}

// Opens a call that needs this call's transition matrices and nothing else of the scorer: on the context's own stream
// (-> *stream), the previous call's results dropped, the matrices of K categories built (prepare_matrices).  Argument
// checks come before it, in the caller.
inline int begin_matrix_call(cafe_ctx* c, const double* lambdas, const double* multipliers, int K, hipStream_t* stream) {
    HIP_TRY(c, hipSetDevice(c->device));
    *stream = c->stream;
    open_call(c, K, c->stream);
    return prepare_matrices(c, lambdas, multipliers, K, c->stream);
}

// A call failed behind an enqueue: whatever it left in flight is drained (best effort; not when the communicator it began with
// was aborted on the way -- a peer is gone, and what waits for it on the stream may never end), the pinned stage is free again,
// and nothing of the call can be read back.  Every failure return behind an enqueue comes through here.
inline void fail_after_enqueue(cafe_ctx* c, hipStream_t s) {
    const bool aborted = c->last.had_comm && !c->comm;
    if (c->device_ready && !aborted && hipSetDevice(c->device) == hipSuccess) (void)hipStreamSynchronize(s);
    c->upload_pending = false;
    c->last.state = LastCall::kNone;
}

// The gate of the read-backs: what the last call must have left -- its matrices and launches (kScored or kMatricesOnly), or a
// scorer's per-family results (kScored alone; the reference leaves `results` empty / stale on a rejected call,
// gamma_core.cpp:173-179).  CAFE_ERR_STATE otherwise.
enum LastNeed { kCompletedCall, kScorerResults };
inline int require_last(cafe_ctx* c, const char* entry, LastNeed what = kCompletedCall) {
    if (c->last.state == LastCall::kScored || (what == kCompletedCall && c->last.state == LastCall::kMatricesOnly)) return CAFE_OK;
    set_err(c, "%s: %s", entry, c->last.state == LastCall::kBatch ? "the last call was a batch (cafe_score_batch): nothing of it can be read back"
                                : what == kCompletedCall ? "no completed call" : "the last call was rejected (+inf) or no call was made");
    return CAFE_ERR_STATE;
}

// What the last call enqueued has finished (read-backs and diagnostics)
inline int wait_last_call(cafe_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->last.stream));
    return CAFE_OK;
}

// Memory for panels: the caller's workspace_limit, else 80 % of what is free now
inline int panel_budget(cafe_ctx* c, size_t* budget) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    *budget = c->workspace_limit ? c->workspace_limit : (size_t)(free_b * 0.8);
    return CAFE_OK;
}

// Columns per pass of a call that walks the unique families in chunks of whole 128-column tiles: as many as panel_budget
// holds at bytes_per_column, at most all; CAFE_ERR_MEMORY with `what` as the error when not even one tile fits.
// (workspace_budget, cafe_ctx.h, is the other rule: calls that cut a list into batches and keep their workspace.)
inline int column_chunk(cafe_ctx* c, size_t bytes_per_column, const std::string& what, int64_t* cols) {
    size_t budget = 0;
    if (const int rc = panel_budget(c, &budget)) return rc;
    *cols = std::min<int64_t>(c->Fp, (int64_t)(budget / bytes_per_column) / kBN * kBN);
    if (*cols < kBN) { set_err(c, "%s", what.c_str()); return CAFE_ERR_MEMORY; }
    return CAFE_OK;
}

// This call's matrix of the branch above node v in category k: row-major for a leaf, k-major (with its non-zero extents,
// nullptr when they are switched off) for an interior node; and a leaf's observed counts from unique column f0 on
inline const double* leaf_matrix(const cafe_ctx* c, int v, int k) { return c->pool.base + (int64_t)c->slot_of[(size_t)v * c->Kmax + k] * c->pool.stride; }
inline const double* interior_matrix(const cafe_ctx* c, int v, int k) { return c->kpool.base + (int64_t)c->slot_of[(size_t)v * c->Kmax + k] * c->kpool.stride; }
inline const int32_t* interior_extents(const cafe_ctx* c, int v, int k) {
    return c->kpool.ext ? c->kpool.ext + (size_t)c->slot_of[(size_t)v * c->Kmax + k] * c->kpool.ext_blocks * 2 : nullptr;
}
inline const int32_t* leaf_counts(const cafe_ctx* c, int v, int64_t f0) { return c->d_counts + (int64_t)c->leaf_taxon[v] * c->Fp + f0; }

// Unique column -> every family that shares it.  fn(family, column - f0) for the families whose column lies in [f0, f0 + ld)
template <class Fn>
void for_each_family_of_chunk(const cafe_ctx* c, int64_t f0, int64_t ld, Fn&& fn) {
    for (int64_t f = 0; f < c->F_all; ++f) {
        const int64_t u = c->ref_of[f];
        if (u >= f0 && u < f0 + ld) fn(f, u - f0);
    }
}
// ... and for a whole table of `per` values per unique column: dst[family] = src[its column]
template <class T>
void spread_unique(const cafe_ctx* c, const T* src, T* dst, int per = 1) {
    for (int64_t f = 0; f < c->F_all; ++f) std::copy(src + c->ref_of[f] * per, src + (c->ref_of[f] + 1) * per, dst + f * per);
}

}  // namespace cafe
