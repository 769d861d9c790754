/* cafe_mi355x.h -- C ABI of the MI355X-native birth-death likelihood path.
 *
 * Drop-in boundary for ONE path of CAFE5 (Han9527/CAFExp): what a scorer call evaluates,
 *   optimizer_scorer::calculate_score            src/optimizer_scorer.cpp:19
 *     -> model::infer_family_likelihoods         src/core.h:171
 *          base_model::infer_family_likelihoods  src/base_model.cpp:53
 *          gamma_model::infer_family_likelihoods src/gamma_core.cpp:169
 * i.e. matrix_cache::precalculate_matrices (src/matrix_cache.cpp:121), inference_prune
 * (src/core.cpp:133) for every family (and gamma category) and the per-family root reduction.
 * and, for what the reference runs once after the search (estimator::execute, src/execute.cpp:147-180):
 * the prunes of compute_pvalues (cafe_root_max), Pupko's reconstruction (cafe_reconstruct) and the Viterbi branch
 * probabilities (cafe_branch_probabilities).
 * Everything behind this header is hand-written HIP for gfx950; there is no CPU fallback:
 * every entry point fails (non-zero code / NULL + message) when no HIP device is usable.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every pointer it passes and nothing is
 *     retained after a call returns except what cafe_create copies;
 *   - numeric rejection is a VALUE, not an error: cafe_score returns 0 and writes +inf exactly
 *     where the reference returns -log(0) (invalid lambda base_model.cpp:56-60; !can_infer
 *     gamma_core.cpp:175-179; a zero-likelihood category gamma_core.cpp:227-236).  NaN is passed
 *     through; the scorer maps it to +inf (optimizer_scorer.cpp:30);
 *   - structural errors (bad arguments, HIP failures) return a non-zero code; the text is
 *     available from cafe_last_error.  Nothing throws across this boundary;
 *   - one call in flight per context (the reference's scorer calls are sequential).
 *
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md; the C++ classes
 * that wrap this ABI behind the reference's model / optimizer_scorer interfaces live in
 * cafexp_amd/host/.
 */
#ifndef CAFE_MI355X_H
#define CAFE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAFE_ABI_VERSION 3
#define CAFE_MAX_CATEGORIES 32

typedef struct cafe_ctx cafe_ctx;

enum {
    CAFE_OK = 0,
    CAFE_ERR_ARGUMENT = 1,   /* malformed problem / params */
    CAFE_ERR_DEVICE = 2,     /* HIP runtime error or no usable device */
    CAFE_ERR_MEMORY = 3,     /* problem does not fit the device */
    CAFE_ERR_STATE = 4       /* call not valid in the context's state */
};

/* Static part of a scorer's state: replaces what model's constructor captures
 * (src/core.cpp:58-70: tree, families, max sizes, error-model shape) plus the clade
 * traversals the reference redoes per family (clade.cpp:255, gene_family.cpp:36). */
typedef struct cafe_problem {
    int32_t n_nodes;                 /* tree nodes; any order with children before parents; exactly one root */
    const int32_t* parent;           /* [n_nodes] parent index, -1 for the root */
    const double*  branch_length;    /* [n_nodes] clade::get_branch_length(); the root's entry is ignored */
    const int32_t* lambda_index;     /* [n_nodes] 0-based lambda of the branch above the node
                                        (clade::get_lambda_index_map, clade.cpp:154); NULL = all 0 */
    const int32_t* leaf_taxon;       /* [n_nodes] column of `counts` for a leaf, -1 for interior nodes */
    int32_t  n_taxa;
    int64_t  n_families;
    const int32_t* counts;           /* [n_families][n_taxa] gene_family::get_species_size */
    int32_t  max_family_size;        /* M, user_data.cpp:46 */
    int32_t  max_root_family_size;   /* R, user_data.cpp:45 */
    int32_t  n_lambdas;              /* lambda::count() */
    int32_t  single_lambda;          /* 1: single_lambda::is_valid (lambda > 0, lambda.h:58);
                                        0: multiple_lambda::is_valid (none < 0, lambda.cpp:59) */
    int32_t  max_categories;         /* largest K any call will use (1 for the base model) */
    int32_t  n_deviations;           /* error_model::n_deviations(), 0 when no error model */
    int32_t  device;                 /* HIP device ordinal */
    int32_t  flags;                  /* CAFE_FLAG_* */
    size_t   workspace_limit;        /* bytes of HBM the likelihood panels may take; 0 = automatic */
} cafe_problem;

#define CAFE_FLAG_NO_DEDUP 1         /* keep identical families separate (build_reference_list, base_model.cpp:27,
                                        collapses them; values are identical either way) */
#define CAFE_FLAG_NO_SUBTREE_DEDUP 2 /* one panel column per family at every node, instead of one per distinct pattern of
                                        leaf counts under the node (the same sharing as build_reference_list, applied per
                                        subtree; values are identical either way) */
/* Missing cells.  With CAFE_FLAG_MISSING_COUNTS set, a cell of `counts` may hold CAFE_COUNT_MISSING: the species' count for that
 * family is unknown and is summed out.  A missing leaf's factor is EXACTLY 1.0 for every parent size, in every category, with or
 * without an error model (no taps are applied to it): sum_c P[s][c] = 1 over all c >= 0 in the untruncated process, so this is
 * the likelihood of the family on the tree with that leaf removed.  It is NOT the truncated row sum sum_{c <= M} P[s][c].  A
 * family whose cells are all missing is allowed; its value is what the prune then gives (every leaf factor 1).  Any other
 * negative count, and every negative count without the flag, is CAFE_ERR_ARGUMENT.  M and R stay the caller's inputs (compute
 * them from the observed cells).  Identical families still share a column -- the missing pattern is part of a family's
 * identity -- and a context created with the flag whose table has no missing cell behaves exactly as one created without it
 * (the same kernels, the same bits).
 * Contexts whose table has a missing cell are accepted by cafe_score, cafe_score_partial, cafe_family_results, cafe_root_max,
 * cafe_root_posterior, cafe_score_per_family(_lm), cafe_leaf_predictive, cafe_shard_plan(_scaled) and cafe_sharded_*.
 * cafe_leaf_predictive returns for a missing cell the predictive mean and sd of the count given the family's observed species;
 * its p_below, p_obs and p_above are NaN there (nothing was observed), and log_evidence is over the observed cells.
 * cafe_pvalues, cafe_reconstruct, cafe_branch_probabilities, cafe_marginal_reconstruct, cafe_sample_histories,
 * cafe_score_gradient, cafe_branch_scores, cafe_expected_events and cafe_branch_change return CAFE_ERR_STATE ("... the table has missing cells")
 * before anything is enqueued; the context stays usable. */
#define CAFE_FLAG_MISSING_COUNTS 4
#define CAFE_COUNT_MISSING (-1)

enum { CAFE_MODEL_BASE = 0, CAFE_MODEL_GAMMA = 1 };

/* Per scorer call: what prepare_calculation (optimizer_scorer.cpp:54,80,123,161) mutates. */
typedef struct cafe_params {
    int32_t model;                   /* CAFE_MODEL_BASE | CAFE_MODEL_GAMMA */
    const double* lambdas;           /* [n_lambdas] */
    int32_t n_categories;            /* K (gamma); ignored for the base model */
    const double* multipliers;       /* [K] gamma_model::_lambda_multipliers */
    const double* cat_probs;         /* [K] gamma_model::_gamma_cat_probs */
    double  alpha;                   /* gamma shape, only for can_infer's alpha >= 0 test (gamma_core.cpp:128) */
    const float*  prior;             /* [R] root_equilibrium_distribution::compute(j): a FLOAT in the reference */
    const double* error_model;       /* [(M+1)][n_deviations] error_model::get_probs(x), or NULL */
} cafe_params;

/* Optional per-family outputs (host pointers, any may be NULL).
 *   base : family_lnl[f] = max_j(log L_j + log prior_j)      (results[i], base_model.cpp:105)
 *   gamma: category_likelihood[f*K+k] = max_j(L_j prior_j) p_k, family_likelihood[f] = sum_k
 *          (family_info_stash rows, gamma_core.cpp:212-216); failed[f] = 1 where a category's
 *          root vector summed to exactly 0 (gamma_core.cpp:152). */
typedef struct cafe_family_out {
    double*  family_lnl;
    double*  category_likelihood;
    double*  family_likelihood;
    int32_t* failed;
} cafe_family_out;

/* HIP-event timings and work counters of the last cafe_score (measurement). */
typedef struct cafe_stats {
    double ms_total;                 /* whole call, host wall */
    double ms_matrices;              /* K1 bd_matrix_build */
    double ms_prune;                 /* K2 prune_gemm + K3 leaf_gather over all nodes */
    double ms_gemm;                  /* K2 only */
    double ms_reduce;                /* K4 root_reduce */
    double gemm_flops;               /* sum over launches of 2*rows*(M+1)*columns, columns = the distinct subtree patterns the
                                        launch processes: every K tile of those columns.  What the tiles really ran (K2
                                        skips the K tiles outside matrix extent x panel extent): cafe_executed_flops */
    double gemm_bytes;               /* algorithmic bytes of the same launches (P + B read, C written) */
    double gemm_flops_per_family;    /* the same sum with one column per (distinct) family at every node: SURVEY 8d's
                                        per-family figure, what the launches would compute without the sharing */
    int64_t gemm_launches;
    int64_t n_matrices;              /* distinct (lambda_q, t_q) keys built */
    int64_t n_unique_families;
    int64_t n_chunks;
    int64_t matrix_bytes;
    int64_t panel_bytes;
    /* the schedule (fixed at cafe_create): */
    int64_t n_assemble_passes;       /* K3 launches that spread factor panels of de-duplicated children over a parent's columns */
    int64_t n_gather_epilogues;      /* K2 launches that fold a sibling's factor panel into their epilogue instead */
    int64_t n_leaf_passes;           /* K3 launches with leaf children only (cherries, polytomies, error models) */
    double gemm_flops_dense;         /* = gemm_flops */
} cafe_stats;

/* NULL on failure; err (optional, errlen bytes) receives the reason.
 * Supported sizes: matrix order N = max(max_family_size, max_root_family_size) + 1 <= 2048.  Under the reference's size
 * rules (user_data.cpp:45-46) that is a largest family count of at most 1637 (N = 2047); 1638 gives N = 2049, which
 * cafe_create rejects with CAFE_ERR_ARGUMENT ("matrix order ... exceeds 2048").  The reference has no such limit. */
cafe_ctx* cafe_create(const cafe_problem* problem, char* err, size_t errlen);
void      cafe_destroy(cafe_ctx* ctx);
const char* cafe_last_error(const cafe_ctx* ctx);
int       cafe_abi_version(void);

/* One model::infer_family_likelihoods call: writes -lnL (or +inf / NaN, see conventions). */
int cafe_score(cafe_ctx* ctx, const cafe_params* params, double* neg_lnl, const cafe_family_out* out);

/* Several parameter vectors in one call: neg_lnl[g] has the bits cafe_score returns for point g's parameters on a context of
 * the same problem under the same root rule (and, where mus is given, with cafe_set_death_rates(mus[g])), whatever else is in
 * the batch and in whatever order.  The G points go through the matrix build and the prune as G * K categories of one call and
 * part only behind the root panel, so a batch costs little more than one call wherever a call is bound by its launch
 * latencies (small matrix orders), and about G calls where one call already fills the device.  A search that knows which
 * points it may need next (Nelder-Mead: expansion and contractions beside the reflection, the first simplex, a shrink) saves
 * dependent round trips with it.
 *   - a point cafe_score would reject on the host (invalid rates, alpha < 0, a saturated longest branch -- by its own lambdas,
 *     mus and multipliers) gets +inf and costs the others nothing; a batch of only such points launches no kernel.  A point
 *     with a category whose root vector sums to zero gets +inf; NaN stays NaN.
 *   - mus non-NULL on a context without death rates set is CAFE_ERR_STATE (cafe_set_death_rates allocates what two rates need);
 *     the context's own death rates are never changed.
 *   - G * K above the problem's max_categories is CAFE_ERR_ARGUMENT; a context with a communicator attached is CAFE_ERR_STATE
 *     (there is no cafe_sharded form either).  Both are refused before anything is enqueued.  A refused or failed batch, like
 *     a refused or failed cafe_score, leaves nothing of the call before it to read back (the last-call record is cleared).
 *   - afterwards cafe_family_results and every other read-back of a last call return CAFE_ERR_STATE (the categories were
 *     several points'); a following cafe_score is unaffected. */
typedef struct cafe_batch_params {
    int32_t n_points;                /* G >= 1 */
    int32_t model;                   /* CAFE_MODEL_BASE | CAFE_MODEL_GAMMA, one for the batch */
    int32_t n_categories;            /* K of every point (gamma); G*K <= the context's max_categories */
    const double* lambdas;           /* [G][n_lambdas] */
    const double* mus;               /* [G][n_lambdas], or NULL: every point under the context's death rates (or none) */
    const double* multipliers;       /* [G][K]  gamma */
    const double* cat_probs;         /* [G][K]  gamma */
    const double* alpha;             /* [G]     gamma (can_infer's test only) */
    const float*  prior;             /* [R], shared by the batch */
    const double* error_model;       /* shared by the batch, or NULL (as cafe_params) */
} cafe_batch_params;
int cafe_score_batch(cafe_ctx* ctx, const cafe_batch_params* params, double* neg_lnl /* [G] */);

/* The same work for a family shard, without the final host read-back: device_partial must point
 * to 2 doubles of DEVICE memory and receives {sum_f lnL_f, number of rejected/invalid families}
 * (+inf rejection that the host can decide alone is encoded as partial[1] = 1).  The kernels are
 * enqueued on `hip_stream` (a hipStream_t used as given: NULL is HIP's null stream, which is what
 * torch.cuda.current_stream() is by default) and the call returns without synchronising, so that
 * the caller can all-reduce the pair across ranks (RCCL) on the same stream: SURVEY.md 8e. */
int cafe_score_partial(cafe_ctx* ctx, const cafe_params* params, double* device_partial, void* hip_stream);
/* Turns the all-reduced pair into the scorer value: +inf if partial[1] > 0 else -partial[0]; NaN if partial[1] is NaN --
 * the mark of a shard whose call FAILED (cafe_score_partial returned an error: it then leaves {0, NaN} in its pair, best
 * effort, so that every rank of the caller's reduction learns of it). */
double cafe_finish_partial(const double host_partial[2]);

/* ---- Multi-GPU: families shard across the GPUs of a node, every GPU builds all matrices, and ONE
 * all-reduce (RCCL over xGMI) of the pair {sum lnL, rejects} closes a scorer call.  The reference has no counterpart:
 * its family loops are OpenMP (base_model.cpp:81-107, gamma_core.cpp:201-244).  Two ways to use it:
 *
 * (1) one process per GPU (torchrun, MPI, ...): every rank creates its context over ITS shard of the families (any
 *     partition gives the same -lnL; cafe_shard_plan balances the ranks), rank 0 makes an id with cafe_comm_unique_id
 *     and hands it to the others by whatever channel the launcher offers, and every rank calls cafe_comm_attach.  From
 *     then on cafe_score on every rank ends with ncclAllReduce(pair, 2 doubles, sum) on the context's stream and returns
 *     the WHOLE table's value on every rank; per-family results stay per shard.  Calls are collective: every rank must
 *     make the same sequence of cafe_score calls.  Ranks fail TOGETHER: a rank whose own call fails (HIP error,
 *     allocation, bad argument) still enters the all-reduce, with rejects = NaN, keeps its own error code, and every
 *     other rank returns CAFE_ERR_DEVICE ("another rank ... failed"); a rank that is gone altogether is caught by a
 *     deadline on the wait (environment CAFE_COMM_TIMEOUT_S at attach, default 120 s; <= 0 waits for ever): the waiting
 *     ranks abort their communicator (ncclCommAbort) and return CAFE_ERR_DEVICE.  After an abort the context has no
 *     communicator any more (attach again, or use it on its own). */
#define CAFE_COMM_ID_BYTES 128
int cafe_comm_unique_id(char id[CAFE_COMM_ID_BYTES]);
int cafe_comm_attach(cafe_ctx* ctx, const char id[CAFE_COMM_ID_BYTES], int32_t world_size, int32_t rank);
int cafe_comm_detach(cafe_ctx* ctx);

/* Balanced family partition for n_shards GPUs.  The device's unit of work is the DISTINCT pattern of leaf counts under
 * an interior node (cafe_create shares likelihood columns between families that agree on a whole subtree), so families
 * are ordered to put look-alikes next to each other (total size, then lexicographically) and cut into consecutive runs
 * of equal predicted device time.  order[n_families]: family indices in shard order; bounds[n_shards + 1]: shard r owns
 * order[bounds[r] .. bounds[r+1]).  Pure host code (no device needed); deterministic, so every rank derives the same
 * plan.  Only tree, counts and max sizes of `problem` are read. */
int cafe_shard_plan(const cafe_problem* problem, int32_t n_shards, int64_t* order, int64_t* bounds);
/* The same with a measured correction: family_scale[n_families] (table order), each in (0.1, 10).  After a few calls under
 * a first plan every rank knows how long its shard took; scale = that time / the mean over the ranks, for every family of
 * the shard, and the plan made with it moves the cuts so that the shards that ran long get less (what the prediction cannot
 * see -- how many K tiles a column's zero extent leaves at this lambda -- is in the measurement).  NULL: cafe_shard_plan. */
int cafe_shard_plan_scaled(const cafe_problem* problem, int32_t n_shards, const double* family_scale, int64_t* order, int64_t* bounds);

/* (2) one process, several GPUs: cafe_create_sharded plans the shards (cafe_shard_plan), creates one context per device
 *     of `devices` -- each driven by its own host thread and stream -- and joins them in one communicator
 *     (ncclCommInitAll).  cafe_sharded_score = model::infer_family_likelihoods over the whole table: all devices
 *     prune their shard concurrently, one all-reduce, one value.  problem->device is ignored. */
typedef struct cafe_sharded cafe_sharded;
cafe_sharded* cafe_create_sharded(const cafe_problem* problem, const int32_t* devices, int32_t n_devices, char* err, size_t errlen);
void      cafe_sharded_destroy(cafe_sharded* s);
const char* cafe_sharded_last_error(const cafe_sharded* s);
int cafe_sharded_score(cafe_sharded* s, const cafe_params* params, double* neg_lnl, const cafe_family_out* out);
/* per-family results of the last call, in the problem's family order (gathered from the shards) */
int cafe_sharded_family_results(cafe_sharded* s, const cafe_family_out* out);
int32_t cafe_sharded_size(const cafe_sharded* s);
/* shard r's context (owned by s): statistics, introspection */
cafe_ctx* cafe_sharded_context(cafe_sharded* s, int32_t r);

/* Per-family results of the last call (valid after the stream was synchronised).  CAFE_ERR_STATE when the last call was
 * no scorer call, was rejected (+inf) or returned an error: a call reported as failed leaves nothing to read back. */
int cafe_family_results(cafe_ctx* ctx, const cafe_family_out* out);

/* P-value path.  For every family of the context: max_j L_root[j], the "observed max likelihood"
 * of compute_tree_pvalue (probability.cpp:391-399) and, on a context holding simulated families, the entries of
 * get_random_probabilities (probability.cpp:273-317, before its sort).  As in the reference the prune uses the
 * plain lambdas (one category, no multiplier), no error model and no prior: params->lambdas is the only field
 * read.  out[n_families].  cafe_family_results is not meaningful after this call. */
int cafe_root_max(cafe_ctx* ctx, const cafe_params* params, double* out);

/* compute_pvalues (probability.cpp:418-454) with the Monte-Carlo simulation on the device as well: n_simulations
 * families per root size 0..R-1 drawn from the transition-matrix rows (set_weighted_random_family_size, :320-351)
 * by a counter-based generator keyed by `seed`, pruned, sorted; pvalues[n_families] = max over root sizes of the
 * upper_bound position (:379-407).  Same distribution as the reference's procedure, a different random sample: agrees
 * with it to Monte-Carlo error, not draw for draw (the host path cafexp_amd/host/pvalues.cpp does the latter).
 * params->lambdas is the only field read; 1 <= n_simulations <= 2048. */
int cafe_pvalues(cafe_ctx* ctx, const cafe_params* params, int32_t n_simulations, uint64_t seed, double* pvalues);

/* Gene-family simulation (the reference's -s: simulator::simulate_processes, src/simulator.cpp:62-103, with
 * set_weighted_random_family_size / adjust_for_error_model, src/probability.cpp:320-377).  Families are simulated down
 * the tree from the given root sizes: every child size is drawn from row `parent size` of the branch's transition matrix
 * (order S = max_family_size, quantized key (lambda * multiplier, t) as matrix_cache_key), restricted to sizes 0..S-1; a
 * parent of size 0 gives 0; an all-zero row (saturated or degenerate branch) gives 0.  Family f belongs to chunk
 * f / chunk_size, whose lambdas are lambdas[i] * chunk_multiplier[chunk] (LAMBDA_PERTURBATION_STEP_SIZE; gamma_core.cpp:88).
 * With an error model, a leaf of size c draws u and becomes c-1 if u < probs[0], c+1 if u > 1 - probs[2]
 * (probs = error_model[c * n_deviations ..]); c >= error_model_max_size fails with CAFE_ERR_ARGUMENT and the reference's
 * message.  The draws come from Philox4x32-10 keyed by `seed` with counter (family, node, stream): the result depends on
 * the arguments only -- not on workspace_limit, batching or device -- and is a different sample than the reference's
 * engine would give (cafexp_amd/host/simulator.cpp follows the reference draw for draw).
 * Chunks whose quantized keys agree share their matrices; the chunks are processed in batches whose matrices and
 * buffers fit workspace_limit bytes (0 = automatic; a batch always holds at least one chunk's matrices). */
typedef struct cafe_sim_problem {
    int32_t n_nodes;                 /* tree nodes; any order with children before parents; exactly one root */
    const int32_t* parent;           /* [n_nodes] parent index, -1 for the root */
    const double*  branch_length;    /* [n_nodes]; the root's entry is ignored */
    const int32_t* lambda_index;     /* [n_nodes] 0-based lambda of the branch above the node; NULL = all 0 */
    const int32_t* leaf_taxon;       /* [n_nodes] column of leaf_counts for a leaf, -1 for interior nodes */
    int32_t  n_taxa;
    int32_t  n_lambdas;
    const double* lambdas;           /* [n_lambdas]: one lambda > 0, or several >= 0 (lambda.h:58, lambda.cpp:59) */
    int32_t  max_family_size;        /* S, 2..2048: sizes 0..S-1 (100 without -f, 2 * max root size with -f) */
    int64_t  n_families;
    const int32_t* root_size;        /* [n_families], each 0..S-1 */
    int32_t  chunk_size;             /* families per lambda multiplier (50 in the reference); 0 = one chunk */
    const double* chunk_multiplier;  /* [ceil(n_families / chunk_size)] >= 0, or NULL = all 1 */
    int32_t  n_deviations;           /* >= 3 with an error model (only probs[0] and probs[2] are read) */
    const double* error_model;       /* [S][n_deviations] error_model::get_probs(c), or NULL */
    int32_t  error_model_max_size;   /* error_model::get_max_family_size(): leaf sizes >= it fail */
    int32_t  device;                 /* HIP device ordinal */
    size_t   workspace_limit;        /* bytes of device memory a batch may take; 0 = automatic */
} cafe_sim_problem;
/* leaf_counts[n_families][n_taxa] and node_sizes[n_families][n_nodes] (host memory; either may be NULL, not both). */
int cafe_simulate(const cafe_sim_problem* problem, uint64_t seed, int32_t* leaf_counts, int32_t* node_sizes, char* err, size_t errlen);
/* The same under separate birth and death rates: mus[n_lambdas], the death rate of the branches of lambda index i (birth rate
 * problem->lambdas[i]); NULL is exactly cafe_simulate.  With mus the order-S matrices of every block are built by the two-rate
 * instantiation of K1 (bd_matrix_lm.hip) from the key (lambda * multiplier, mu * multiplier, t) -- a chunk multiplier scales both rates, as
 * gamma multipliers do everywhere else -- and chunks share their matrices when both quantized vectors agree.  The row sums, the
 * sampler, the Philox counters, the error-model step and the batching are cafe_simulate's.  Every mu must be finite, >= 0 and
 * mu * multiplier * 1e9 within the bound lambda has: CAFE_ERR_ARGUMENT with a message that names mu otherwise.  With
 * mus[i] == lambdas[i] the output is cafe_simulate's for the same seed. */
int cafe_simulate_lm(const cafe_sim_problem* problem, const double* mus, uint64_t seed, int32_t* leaf_counts, int32_t* node_sizes,
                     char* err, size_t errlen);

/* model::infer_family_likelihoods for ONE family at a time, each with its own lambdas (estimate_lambda_per_family,
 * execute.cpp:104-128).  family[n] indexes the context's families (caller's order, duplicates allowed);
 * lambdas[n][n_lambdas].  family_lnl[n] receives what cafe_score's family_lnl[family[i]] would be with
 * params->lambdas = lambdas[i]: -inf where cafe_score would return +inf for that vector (invalid lambda, zero
 * likelihood), NaN passed through.  Base model only (CAFE_MODEL_GAMMA: CAFE_ERR_ARGUMENT; a context with a communicator
 * attached: CAFE_ERR_STATE); params->prior and params->error_model are read, params->lambdas is not.  No matrix is built
 * in memory: one wave per (family, branch) runs the row recurrence and consumes every row in a dot product
 * (family_lambda.hip).  The list is processed in batches that fit the problem's workspace_limit (0 = automatic); a value
 * depends on the family's counts and lambdas only, never on the list or the batches.  cafe_family_results is not
 * meaningful after this call. */
int cafe_score_per_family(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family,
                          const double* lambdas, double* family_lnl);
/* The same with separate birth and death rates PER FAMILY: lambdas[n][n_lambdas] and mus[n][n_lambdas], entry i scores
 * family[i] under its own pair.  Everything else is cafe_score_per_family's: base model only, params->prior and
 * params->error_model are read, the list is processed in batches that fit workspace_limit, a value depends on the family's
 * counts and its rates only, CAFE_ERR_STATE with a communicator attached.  The context's own death rates
 * (cafe_set_death_rates) are NOT read: the call is valid, and gives the same values, whether or not they are set.
 * Validity per entry is the context's rule as cafe_set_death_rates applies it -- one lambda: lambda > 0; several: no lambda
 * negative; every mu must satisfy mu >= 0 (so a NaN mu is invalid, as it is in the setter's calls) -- and an invalid entry gives
 * -inf; a NaN lambda that passes the rule gives NaN.  Either rate * 1e9 beyond a long gives the saturated branch (rows >= 1
 * zero), as a lambda beyond it does in cafe_score_per_family.  The branch kernel is that entry's, instantiated for two rates
 * (family_lambda_kernel.h: the row step of bd_row.h on the key (lambda, mu, t), quantized like cafe_bd_rates); with
 * mus[i] == lambdas[i] every value is bit for bit what cafe_score_per_family returns for that vector. */
int cafe_score_per_family_lm(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family,
                             const double* lambdas, const double* mus, double* family_lnl);

/* The per-family path under a gene GAIN rate: n -> n+1 at rate n lambdas + nus, n -> n-1 at rate n mus (the linear birth-death
 * process with immigration; size 0 is no longer absorbing, so a family absent in an ancestor can appear below it).  Entry i
 * scores family[i] under (lambdas[i], mus[i], nus[i]), each [n_lambdas]; mus == NULL means mu = lambda.  The single-lineage law
 * and its alpha and beta are cafe_bd_rates'; row s of a branch's matrix is row s-1 convolved with that law as before, and row 0
 * is the law of the immigrants' descendants, cafe_bd_gain_row0.  The root's size runs over 0..R: size 0 has prior mass
 * root_absent, size j >= 1 has (1 - root_absent) * prior[j-1], under the context's root rule (cafe_set_root_rule).
 * family[i] == CAFE_FAMILY_ABSENT scores the profile with every species' count 0 under entry i's rates, whether or not the
 * table holds such a family (with an error model: the taps of an observed 0) -- what a likelihood conditional on the family
 * having been seen needs.  Everything else is cafe_score_per_family_lm's contract: base model only, CAFE_ERR_STATE with a
 * communicator attached, the context's death rates are not read, an invalid entry gives -inf and a NaN lambda that passes the
 * rule gives NaN, a rate * 1e9 beyond a long saturates the branch.  A nu that is negative or NaN, or root_absent outside
 * [0, 1], is CAFE_ERR_ARGUMENT.  With nus all 0 and root_absent = 0 every value is bit for bit cafe_score_per_family_lm's
 * (cafe_score_per_family's with mus == lambdas or NULL). */
#define CAFE_FAMILY_ABSENT (-1)   /* the profile with every species' count 0, whether or not the table holds it */
int cafe_score_per_family_gain(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family,
                               const double* lambdas, const double* mus, const double* nus, double root_absent, double* family_lnl);
/* Row 0 of the gain model's matrix for the key (lambda, mu, nu, t): the three rates quantized like a lambda, t like a branch
 * length, alpha and beta cafe_bd_rates'.  out[k] = C(r+k-1, k) (1-beta)^r beta^k, k < n, r = nu / lambda (written to out_r[0]
 * unless out_r is NULL; +inf for lambda = 0 < nu).  nu = 0 gives exactly e_0.  lambda = 0 < nu is the limit r -> inf, beta -> 0:
 * the Poisson law with mean nu (1 - exp(-mu t)) / mu (nu t for mu = 0).  The kernel evaluates the same formula.  Pure host code,
 * no device needed.  CAFE_ERR_ARGUMENT for a negative or NaN argument or a rate * 1e9 beyond a long. */
int cafe_bd_gain_row0(double lambda, double mu, double nu, double t, int32_t n, double* out, double out_r[1]);

/* Posterior absence, origin and loss under the gain model: for entry i -- family[i] under (lambdas[i], mus[i], nus[i]), as in
 * cafe_score_per_family_gain, whose arguments these are and whose checks apply (base model only; an error model, missing cells
 * and CAFE_FAMILY_ABSENT are accepted; CAFE_ERR_STATE with a communicator attached; a negative or NaN nu, or root_absent
 * outside [0, 1], is CAFE_ERR_ARGUMENT) -- and every node v of the tree,
 *   p_absent   P(size(v) = 0 | counts)
 *   mean       the posterior mean of size(v)
 *   p_gain     P(size(parent(v)) = 0, size(v) >= 1 | counts): the family originated on the branch above v.  NaN at the root
 *   p_loss     P(size(parent(v)) >= 1, size(v) = 0 | counts): the family was lost on that branch.  NaN at the root
 *   posterior  the whole distribution of size(v), cafe_matrix_size values per node, 0 past the node's range; NULL: not wanted
 *              (one batch of it is staged in host memory: ask for it on short family lists)
 *   lnl        the family's lnL; NULL: not wanted
 * Root sizes run over 0..R with mass root_absent at 0 and (1 - root_absent) * (double)prior[j-1] at j; the other nodes' sizes
 * over 0..M.  A posterior is a ratio against the marginal likelihood, so the call uses the SUM rule always: it neither reads nor
 * changes cafe_set_root_rule, and lnl is bit for bit cafe_score_per_family_gain's under CAFE_ROOT_SUM.  Every output is
 * divided by the family's Z = exp(lnl).  p_gain and p_loss are computed as sums of their own, not as differences.
 * A MISSING leaf has factor exactly 1.0 -- the row sums of the untruncated process -- and is normalised by the same Z: its
 * p_absent and p_gain are those of the untruncated process (p_gain from 1 - P[0][0] of cafe_bd_gain_row0), its mean and
 * posterior run over 0..M only, so its posterior sums to 1 less the mass the process puts past M.  Every other node's
 * posterior sums to 1.
 * An entry whose rates are invalid has lnl = -inf, one whose rates are NaN has lnl = NaN (cafe_score_per_family_gain's rule),
 * and both have NaN in every other output; so has a family whose lnl from the device is not finite.  Arrays are indexed
 * [entry][node] ([entry][node][size] for posterior) in the node order of cafe_problem.  A later cafe_score returns what it
 * returned before the call. */
typedef struct cafe_gain_posterior_out {
    double* lnl;        /* [n]           sum-rule lnL of the family; may be NULL */
    double* p_absent;   /* [n][n_nodes]  P(size(node) = 0 | counts) */
    double* mean;       /* [n][n_nodes]  posterior mean size of the node */
    double* p_gain;     /* [n][n_nodes]  P(size(parent) = 0, size(node) >= 1 | counts); NaN at the root */
    double* p_loss;     /* [n][n_nodes]  P(size(parent) >= 1, size(node) = 0 | counts); NaN at the root */
    double* posterior;  /* optional, NULL or [n][n_nodes][cafe_matrix_size]: the whole distribution, 0 past the node's range */
} cafe_gain_posterior_out;
int cafe_gain_posterior(cafe_ctx* ctx, const cafe_params* params, int64_t n, const int64_t* family, const double* lambdas,
                        const double* mus, const double* nus, double root_absent, const cafe_gain_posterior_out* out);

/* Separate birth and death rates.  The reference fits the critical process lambda = mu only; with death rates set a context
 * scores the linear birth-death process with birth rate lambdas[i] and death rate mus[i] per lineage on the branches of
 * lambda index i.  mus[n_lambdas] is copied; NULL restores lambda = mu (and the kernels that run then).  While death rates
 * are set every call that builds transition matrices uses them: cafe_score, cafe_score_partial, cafe_root_max,
 * cafe_reconstruct, cafe_branch_probabilities, cafe_marginal_reconstruct, cafe_pvalues (its own order-S matrices and its
 * simulated families' prune included) and with them cafe_get_matrix / cafe_get_extents.  Gamma multipliers scale both rates.
 * Validity follows the context's rule for lambdas -- one lambda: lambda > 0 and mu >= 0; several: none negative -- and an
 * invalid mu makes a call's value +inf (or its error) exactly as an invalid lambda does; the gamma model's host rejection
 * (gamma_core.cpp:131-139) reads coeff = 1 - alpha - beta of the longest branch under the largest of either rate.  With
 * mus[i] == lambdas[i] every result is bit for bit the unset call's.
 * cafe_score_per_family returns CAFE_ERR_STATE while death rates are set (its kernel is the lambda = mu row step):
 * cafe_score_per_family_lm takes the death rates per family and does not read the context's.  cafe_simulate, which takes no
 * context, simulates lambda = mu; cafe_simulate_lm takes the death rates as an argument.  Sharded use needs no entry of its own:
 * call the setter on every cafe_sharded_context(s, r) (or on every rank's context) before the collective call. */
int cafe_set_death_rates(cafe_ctx* ctx, const double* mus);
/* What a transition matrix is built from, for the key (lambda, mu, t): lambda and mu quantized like lambda, t like the branch
 * length (matrix_cache_key, matrix_cache.h:42-61).  out[0] = alpha = P(a lineage is extinct after t), out[1] = beta, the ratio
 * of the geometric tail p1(k) = (1-alpha)(1-beta) beta^(k-1),
 *     alpha = mu (E-1) / (lambda E - mu),   beta = lambda (E-1) / (lambda E - mu),   E = exp((lambda - mu) t),
 * evaluated through expm1 and exp(-|lambda-mu| t) so that both are finite and below 1 for every valid key and tend to
 * lambda t / (1 + lambda t) as mu -> lambda; equal quantized rates give exactly the bits the lambda = mu kernels use.
 * out[2] = 1 when the matrix is built with rows s >= 1 all zero: !(coeff > 0 && coeff != 1), coeff = 1 - alpha - beta.  That
 * is the reference's saturation rule (matrix_cache.cpp:153, probability.cpp:154) carried over so that the model is continuous
 * at mu = lambda and lambda = mu = 0 stays degenerate -- a convention: the recurrence itself is defined wherever alpha and
 * beta are below 1.  Pure host code, no device needed. */
int cafe_bd_rates(double lambda, double mu, double t, double out[3]);

/* Ancestral reconstruction.  Pupko's joint reconstruction as reconstruct_gene_family runs it
 * (gene_family_reconstructor.cpp:13-165; base_model.cpp:145, gamma_core.cpp:301): for every category k (one for
 * the base model; lambda * multipliers[k] for the gamma model) and family f, the reconstructed size of every node
 * -> states[k][f][node] (leaves carry their observed counts).  root_prior[j] = root_equilibrium_distribution::
 * compute(j) for j = 0..min(M,R) (one more entry than params->prior: the root scan of :47-62 reads compute(j) with
 * j as the SIZE, up to min(M,R) inclusive).  No error model is applied (:28-32 read the matrix column of the
 * observed count).  params: model, lambdas, n_categories, multipliers. */
int cafe_reconstruct(cafe_ctx* ctx, const cafe_params* params, const float* root_prior, int32_t* states);
/* compute_viterbi_sum (gene_family_reconstructor.cpp:361-400) for every family and node under the plain lambdas:
 * sizes[f][node] are the (reconstructed / observed) sizes, out[f][node] the branch probability, NaN where the
 * reference returns "invalid" (the root; parent size == child size). */
int cafe_branch_probabilities(cafe_ctx* ctx, const cafe_params* params, const int32_t* sizes, double* out);

/* Marginal ancestral reconstruction under the SCORER's model (inference_prune with the call's lambdas, categories, prior
 * and error model -- not cafe_reconstruct's joint variant): an up pass and a down pass of sum-products give, for every
 * family f and node v, the posterior distribution of the node's size.  With the gamma model the categories are mixed with
 * weights cat_probs[k] before anything is summarised.  Outputs, [n_families][n_nodes] in the problem's orders unless noted
 * (host pointers, any may be NULL):
 *   mean, mode (first arg max), lo / hi: the equal-tailed interval on the discrete CDF at `level` in (0, 1),
 *     lo = min{j : CDF(j) >= (1 - level) / 2}, hi = min{j : CDF(j) >= 1 - (1 - level) / 2};
 *   p_increase / p_decrease = P(X_v > X_parent | data) / P(X_v < X_parent | data) for the branch above v; NaN at the root;
 *   a leaf's row is its observed count, or with an error model the posterior over the model's taps;
 *   log_evidence[n_families] = log Z, Z = sum_k p_k sum_s prior[s-1] B_root[s]; failed[n_families] = 1 where Z is 0 or not
 *     finite: that family's doubles are NaN and its integers -1 (the call still returns CAFE_OK).
 * Reads model, lambdas, n_categories, multipliers, cat_probs, prior and error_model of params.  CAFE_ERR_ARGUMENT for a level
 * outside (0, 1), invalid lambdas or a bad K; CAFE_ERR_STATE on a context with a communicator attached.  The columns are
 * processed in batches that fit the problem's workspace_limit (0 = automatic); a value never depends on the batches.
 * cafe_family_results is not meaningful after this call; a later cafe_score is unaffected. */
typedef struct cafe_marginal_out {
    double*  mean;
    int32_t* mode;
    int32_t* lo;
    int32_t* hi;
    double*  p_increase;
    double*  p_decrease;
    double*  log_evidence;
    int32_t* failed;
} cafe_marginal_out;
int cafe_marginal_reconstruct(cafe_ctx* ctx, const cafe_params* params, double level, const cafe_marginal_out* out);
/* measurement: flops of the GEMM launches of the last cafe_marginal_reconstruct and, when it ran with profiling on
 * (cafe_set_profiling), their summed HIP-event time in milliseconds (else 0) */
int cafe_debug_marginal_gemm(cafe_ctx* ctx, double* ms, double* flops);

/* Ancestral histories drawn from the posterior of the model of cafe_marginal_reconstruct (the scorer's: leaf vectors with
 * the error model's taps, interior sizes 0..M, root sizes 1..R under the float prior, gamma categories): n_draws whole
 * assignments of a size to every node of every family, for statements about several nodes or families at once.  With B the
 * up-pass vector of a node, P its branch's matrix and u(f, v, s) the Philox uniform of (family f, node v, stream s) keyed
 * by `seed`, draw d of family f takes
 *   the category: the first k over cat_probs[k] Z_k, Z_k = sum_s prior[s-1] B_root^k[s], with u(f, root, 2d+1) (0: base model);
 *   the root: the first s in 1..R over prior[s-1] B_root^k[s], with u(f, root, 2d);
 *   a node v whose parent drew i: the first j in 0..M over P_v^k[i][j] B_v^k[j], with u(f, v, 2d) (a parent at 0 gives 0);
 *   a leaf: its observed count, or with an error model the first tap c over err[x][t] P_v^k[i][c], with u(f, v, 2d);
 * "first" = the first index whose inclusive prefix sum is >= u * (sum of all weights); an all-zero range gives its first
 * index.  f is the family's index in the problem's table: identical families draw different histories.  The result is a
 * function of the arguments only (not of workspace_limit, batches or the device).  Outputs (host pointers, any may be NULL):
 *   sizes [n_draws][n_families][n_nodes] and category [n_draws][n_families] in the problem's orders;
 *   n_increase / n_decrease [n_draws][n_nodes]: the families of a draw with X_v > / < X_parent(v); net_change: the sum over
 *     the families of X_v - X_parent(v); 0 at the root.  They are counted on the device: with sizes = NULL nothing of size
 *     n_draws * n_families * n_nodes is moved;
 *   log_evidence, failed [n_families] as cafe_marginal_reconstruct: a failed family (Z = 0 or not finite) has sizes and
 *     category -1 and adds nothing to the counts.
 * Reads model, lambdas, n_categories, multipliers, cat_probs, prior and error_model of params; the context's death rates
 * apply.  CAFE_ERR_ARGUMENT for invalid rates, a bad K or n_draws outside 1..65536; CAFE_ERR_STATE on a context with a
 * communicator attached.  cafe_family_results is not meaningful after this call; a later cafe_score is unaffected. */
typedef struct cafe_history_out {
    int32_t* sizes;
    int32_t* category;
    int64_t* n_increase;
    int64_t* n_decrease;
    int64_t* net_change;
    double*  log_evidence;
    int32_t* failed;
} cafe_history_out;
int cafe_sample_histories(cafe_ctx* ctx, const cafe_params* params, int32_t n_draws, uint64_t seed,
                          const cafe_history_out* out);
/* diagnostics: how the last cafe_sample_histories cut its work under the workspace budget -- the column batches of the
 * unique families and the passes over the draws that each batch took */
int cafe_debug_history_batches(cafe_ctx* ctx, int32_t* column_batches, int32_t* draw_passes);

/* Per-family score vectors: the derivative of every family's log likelihood in the rates, at the call's parameters.  The
 * model, the passes and the GEMM are cafe_marginal_reconstruct's; the branch joint G_v P_v B_v that it forms is contracted
 * with dP_v / d theta through a linear transform of B_v and one more GEMM per interior branch and free rate (no derivative
 * matrix is built).  root_rule chooses what is differentiated:
 *   CAFE_ROOT_MAX  what cafe_score returns per family -- base model: max_s(log L_s + log prior_s), first maximum; gamma model:
 *                  log sum_k p_k max_s(L_s prior_s); the root weight of a category is the prior at its arg max, zero elsewhere;
 *   CAFE_ROOT_SUM  cafe_marginal_reconstruct's log_evidence, Z = sum_k p_k sum_s prior[s-1] B_root[s].
 * Outputs (host pointers, any may be NULL), rows in the problem's family order:
 *   family_lnl[n_families] the differentiated value; failed[n_families] = 1 where Z is 0 or not finite: that family's doubles
 *     are NaN (the call still returns CAFE_OK);
 *   d_lambda[n_families][n_lambdas]: without death rates the derivative along lambda = mu (a non-NULL d_mu is then
 *     CAFE_ERR_STATE); with death rates set d_lambda and d_mu[n_families][n_lambdas] are the two partials, and at mus == lambdas
 *     their sum is the unset call's d_lambda to rounding;
 *   d_multiplier[n_families][K], gamma model only (CAFE_ERR_ARGUMENT otherwise): the derivative in multipliers[k], which
 *     scales both rates of category k; cat_probs are held fixed.
 * The derivative is that of the smooth likelihood at the quantized keys the call builds its matrices from (cafe_bd_rates).  A
 * branch whose key is marked zero (cafe_bd_rates out[2]) contributes 0.  The error model is read, not differentiated.
 * CAFE_ERR_ARGUMENT for invalid rates, a bad K or root_rule; CAFE_ERR_STATE on a context with a communicator attached.  The
 * columns are processed in batches that fit the problem's workspace_limit (0 = automatic); a value never depends on the
 * batches, identical families get identical rows.  cafe_family_results is not meaningful after this call; a later cafe_score
 * is unaffected; cafe_debug_marginal_gemm reports this call's GEMM launches. */
enum { CAFE_ROOT_MAX = 0, CAFE_ROOT_SUM = 1 };
typedef struct cafe_gradient_out {
    double*  family_lnl;    /* [n_families] log Z_f under the chosen root rule */
    double*  d_lambda;      /* [n_families][n_lambdas] */
    double*  d_mu;          /* [n_families][n_lambdas]; only while death rates are set */
    double*  d_multiplier;  /* [n_families][K]; gamma model only */
    int32_t* failed;        /* [n_families] */
} cafe_gradient_out;
int cafe_score_gradient(cafe_ctx* ctx, const cafe_params* params, int32_t root_rule, const cafe_gradient_out* out);
/* out = {d alpha / d lambda, d alpha / d mu, d beta / d lambda, d beta / d mu} of cafe_bd_rates' alpha and beta at the same
 * quantized key.  Evaluated without a division by lambda - mu (expm1 away from it, a series where |lambda - mu| t is small), so
 * finite and accurate as mu -> lambda; at equal quantized rates the four limits, whose sums out[0] + out[1] and out[2] + out[3]
 * both equal t / (1 + lambda t)^2, the derivative of the lambda = mu kernels' alpha.  Pure host code, no device needed. */
int cafe_bd_rates_grad(double lambda, double mu, double t, double out[4]);

/* Per-branch scores for a rate-shift scan: cafe_score_gradient's derivative kept per branch, and the information of those
 * scores.  For every family f and non-root node v, with c_v a factor on BOTH rates of the branch above v (and on nothing
 * else), rate[f][v] = d lnL_f / d log c_v at c = 1; since the matrix of a branch depends on it only through lambda t and mu t,
 * that is also t_v d lnL_f / d t_v.  With death rates set, birth and death are the same for a factor on lambda alone and on mu
 * alone, rate = birth + death; without them birth / death non-NULL is CAFE_ERR_STATE.  The model, the two passes, the root
 * rules, the column batches and the error codes are cafe_score_gradient's; with the gamma model the categories mix as there:
 * a branch's score is sum_k of the category's weight times (lambda_q m_k d/d(lambda_q m_k) + mu_q m_k d/d(mu_q m_k)) restricted
 * to that branch.  The derivative is that of the smooth likelihood at the quantized keys; a zero-marked branch (cafe_bd_rates
 * out[2]) gives exactly 0.  Sums: over the branches of lambda index q, rate (birth) adds up to lambdas[q] d_lambda[q], death to
 * mus[q] d_mu[q]; over all branches rate adds up to sum_k multipliers[k] d_multiplier[k] -- to rounding.
 * family_lnl, d_lambda, d_mu, d_multiplier and failed are bit for bit cafe_score_gradient's for the same arguments (one body).
 * The score vector z_f has P = cafe_branch_scores_dim entries: without death rates `rate` of every non-root node in the
 * problem's node order; with death rates `birth` of every non-root node, then `death` of every non-root node; then d_lambda
 * [n_lambdas], d_mu [n_lambdas] while death rates are set, d_multiplier [K] under the gamma model.  total = sum_f z_f and
 * gram = sum_f z_f z_f^T over the families that did not fail (n_used of them), formed on the device once, after the last
 * column batch, from the scores of all distinct families weighted by their multiplicity (cafe_weighted_gram): neither depends
 * on workspace_limit, and gram is exactly symmetric.  The panel of those scores -- P x (distinct families, padded to 128)
 * doubles -- stays on the device beside one batch and is not counted against workspace_limit; CAFE_ERR_MEMORY when it does not
 * fit.  A failed family (Z = 0 or not finite) has NaN doubles in its rows, failed = 1, and adds nothing to total / gram.  The
 * root's entries of rate / birth / death are NaN.  Any pointer may be NULL; with gram, total, n_used NULL no Gram is formed, and
 * with the [n_families][n_nodes] pointers NULL nothing of that size leaves the device.  cafe_debug_marginal_gemm reports this
 * call's GEMM launches: the same as cafe_score_gradient's. */
typedef struct cafe_branch_scores_out {
    double*  rate;         /* [n_families][n_nodes] d lnL_f / d log c_v, c_v scaling BOTH rates of the branch above v; NaN at the root */
    double*  birth;        /* [n_families][n_nodes] d / d log lambda_v; only while death rates are set (else CAFE_ERR_STATE) */
    double*  death;        /* [n_families][n_nodes] d / d log mu_v;     likewise; rate = birth + death */
    double*  family_lnl;   /* as cafe_gradient_out */
    double*  d_lambda;
    double*  d_mu;
    double*  d_multiplier; /* as cafe_gradient_out, from the same pass */
    int32_t* failed;
    double*  total;        /* [P]    U = sum_f z_f over the families that did not fail */
    double*  gram;         /* [P][P] sum_f z_f z_f^T, row-major, exactly symmetric */
    int64_t* n_used;       /* families that entered total / gram */
} cafe_branch_scores_out;
int cafe_branch_scores(cafe_ctx* ctx, const cafe_params* params, int32_t root_rule, const cafe_branch_scores_out* out);
/* P, the length of the score vector, for this context's death rates and params->model / n_categories */
int cafe_branch_scores_dim(const cafe_ctx* ctx, const cafe_params* params, int32_t* P);
/* measurement: the flops of the MFMAs of the Gram kernel of the last cafe_branch_scores (lower-triangle tiles only) and, when
 * it ran with profiling on (cafe_set_profiling), the HIP-event time in milliseconds of its three launches (else 0) */
int cafe_debug_gram(cafe_ctx* ctx, double* ms, double* flops);

/* Expected gene gains and losses: the posterior expectation, given the leaf counts, of the number of births (gains) and of
 * deaths (losses) on the branch above every node -- the turnover that node sizes do not show (a branch on which a family gained
 * three genes and lost three has no net change).  The model is cafe_marginal_reconstruct's: the call's lambdas, categories,
 * prior and error model, the context's death rates when set, the root weight of CAFE_ROOT_SUM; with the gamma model the
 * categories mix with their posterior weights.  Tagging every birth with a factor r and every death with w keeps the
 * single-lineage law linear-fractional, and the expected counts are the derivatives in r and w at 1 of the branch's matrix,
 * contracted with the branch joint as cafe_score_gradient does: two scans of B_v in one pass, two GEMMs and two weighted dots
 * per interior branch, no derivative matrix.  Outputs (host pointers, any may be NULL), rows in the
 * problem's family order:
 *   gains, losses [n_families][n_nodes]: NaN at the root; gains - losses is the posterior mean of X_v - X_parent(v).  The events
 *     of a leaf branch are those leading to the true size behind the error model's taps;
 *   log_evidence, failed [n_families] as cafe_marginal_reconstruct: a failed family's doubles are NaN (the call still returns
 *     CAFE_OK).
 * A branch whose key is marked zero (cafe_bd_rates out[2]) contributes 0.  CAFE_ERR_ARGUMENT for invalid rates or a bad K;
 * CAFE_ERR_STATE on a context with a communicator attached.  The columns are processed in batches that fit the problem's
 * workspace_limit (0 = automatic); a value never depends on the batches, identical families get identical rows.
 * cafe_family_results is not meaningful after this call; a later cafe_score is unaffected; cafe_debug_marginal_gemm reports this
 * call's GEMM launches. */
typedef struct cafe_events_out {
    double*  gains;        /* [n_families][n_nodes] E[births on the branch above v | data]; NaN at the root */
    double*  losses;       /* [n_families][n_nodes] E[deaths on the branch above v | data]; NaN at the root */
    double*  log_evidence; /* [n_families] */
    int32_t* failed;       /* [n_families] */
} cafe_events_out;
int cafe_expected_events(cafe_ctx* ctx, const cafe_params* params, const cafe_events_out* out);
/* out = {da, db, dc} of the births tag, then {da, db, dc} of the deaths tag, at r = w = 1 and the quantized key of cafe_bd_rates:
 * the derivatives of the tagged law phi(z) = a + c z / (1 - b z), whose a and b are cafe_bd_rates' alpha and beta and whose
 * c = (1 - alpha)(1 - beta) there.  All six are non-negative; evaluated without a division by lambda - mu (series where
 * |lambda - mu| t is small), so finite and accurate as mu -> lambda and at mu = lambda.  Pure host code, no device needed. */
int cafe_bd_rates_events(double lambda, double mu, double t, double out[6]);

/* Leave-one-out predictive check of every leaf count: the distribution of species l's count given the counts of every other
 * species of the family, under cafe_marginal_reconstruct's model (the call's lambdas, categories, prior and error model, the
 * context's death rates when set, the root weight of CAFE_ROOT_SUM).  With G_l the down pass's outside message on the parent's
 * sizes (O_parent times the siblings' factors) and P_l the leaf's matrix,
 *     O_l[c] = sum_i P_l[i][c] G_l[i], c = 0..M        u = sum_k p_k O_l^k
 *     w[y] = u[y], or with an error model sum_t err[y][t] u[y - half + t] (taps outside [0, M] dropped)        W = sum_y w[y]
 * so that w[x] at the observed count x is the family's evidence Z and nothing else in w depends on x.  One fp64 MFMA GEMM per
 * leaf branch and category forms O_l for all columns; the sums over y follow in a second kernel.  Outputs
 * (host pointers, any may be NULL), rows in the problem's family order, columns as `counts`:
 *   mean, sd [n_families][n_taxa]: of w / W over 0..M; they do not depend on x, not even in the last bit;
 *   p_below, p_obs, p_above: the mass of y < x, y = x and y > x, each summed on its own (a small tail keeps its relative
 *     accuracy); p_below + p_obs and p_obs + p_above are the two one-sided tail probabilities of the observed count;
 *   log_evidence, failed [n_families] as cafe_marginal_reconstruct, judged on Z.
 * A cell whose W is zero or not finite has NaN in all five (the call still returns CAFE_OK); a family that failed because its
 * observation is impossible may still have finite cells with p_obs = 0.  CAFE_ERR_ARGUMENT for invalid rates or a bad K;
 * CAFE_ERR_STATE on a context with a communicator attached.  The columns are processed in batches that fit the problem's
 * workspace_limit (0 = automatic); a value never depends on the batches, identical families get identical rows.
 * cafe_family_results is not meaningful after this call; a later cafe_score is unaffected; cafe_debug_marginal_gemm reports this
 * call's GEMM launches. */
typedef struct cafe_leaf_predictive_out {
    double*  mean;          /* [n_families][n_taxa], columns as `counts` */
    double*  sd;
    double*  p_below;
    double*  p_obs;
    double*  p_above;
    double*  log_evidence;  /* [n_families] */
    int32_t* failed;        /* [n_families] */
} cafe_leaf_predictive_out;
int cafe_leaf_predictive(cafe_ctx* ctx, const cafe_params* params, const cafe_leaf_predictive_out* out);

/* Posterior of each branch's size change: for every family and non-root node v, the distribution of Delta = X_v - X_parent(v)
 * given the leaf counts -- by how much the family changed on the branch, and how sure that is.  Parent and child are strongly
 * correlated, so this cannot be formed from the two nodes' rows of cafe_marginal_reconstruct.  The model is that call's: the
 * call's lambdas, categories, prior and error model, the context's death rates when set, the root weight of CAFE_ROOT_SUM.  With
 * G_v the down pass's outside message on the parent's sizes, P_v the branch's matrix and B_v the up pass's message of v, per
 * category k (i = 0..np, np = R under the root, else M; j = 0..M; P[0][j] = delta(j, 0)):
 *     J_k[i][j] = G_v^k[i] P_v^k[i][j] B_v^k[j]
 *     w[d]  = sum_k p_k sum_i J_k[i][i + d],  d = -max_change..max_change, terms with i + d outside 0..M absent
 *     below = sum_k p_k sum_{j - i < -max_change} J_k[i][j]        above = sum_k p_k sum_{j - i > max_change} J_k[i][j]
 * all divided by Z = sum_k p_k Z_k.  A leaf branch without an error model has j fixed at the observed x; with one, Delta is
 * (true size c_t) - i with weights err[x][t] G[i] P[i][c_t], the taps in the scorer's order, taps outside 0..M dropped.  Each
 * w[d] is summed in the order of i, then over the taps, then over k: it has the same bits whatever max_change, workspace_limit
 * or column batch the call ran with.  The tails are sums of their own, never complements.  Outputs (host pointers, any may
 * be NULL), in the problem's orders:
 *   pmf [n_families][n_nodes][2 max_change + 1]: P(Delta = d | data), d ascending;
 *   below, above [n_families][n_nodes]: P(Delta < -max_change | data), P(Delta > max_change | data);
 *   mean [n_families][n_nodes] = E[X_v] - E[X_parent] from the two nodes' posteriors: exact over the whole range, not the band's;
 *   mode: the first arg max over the band;  lo / hi: the equal-tailed interval at `level` in (0, 1) on the CDF over
 *     (below, -max_change..max_change, above): lo = min{d : CDF(d) >= (1 - level) / 2}, hi = min{d : CDF(d) >= 1 - (1 - level) / 2};
 *     lo = -max_change - 1 / hi = max_change + 1: the crossing lies in the lower / upper tail (raise max_change);
 *   log_evidence, failed [n_families] as cafe_marginal_reconstruct.
 * At the root, and at every node of a failed family (Z zero or not finite), the doubles are NaN and the integers
 * CAFE_CHANGE_NONE (-1 is a valid change); the call still returns CAFE_OK.  CAFE_ERR_ARGUMENT for max_change outside
 * 0..max(M, R), a level outside (0, 1), invalid rates or a bad K; CAFE_ERR_STATE on a context with a communicator attached or
 * with missing cells.  The columns are processed in batches that fit the problem's workspace_limit (0 = automatic); identical
 * families get identical rows.  cafe_family_results is not meaningful after this call; a later cafe_score is unaffected;
 * cafe_debug_marginal_gemm reports this call's GEMM launches. */
#define CAFE_CHANGE_NONE (-2147483647 - 1)
typedef struct cafe_branch_change_out {
    double*  pmf;           /* [n_families][n_nodes][2 max_change + 1] */
    double*  below;         /* [n_families][n_nodes] */
    double*  above;
    double*  mean;
    int32_t* mode;
    int32_t* lo;
    int32_t* hi;
    double*  log_evidence;  /* [n_families] */
    int32_t* failed;        /* [n_families] */
} cafe_branch_change_out;
int cafe_branch_change(cafe_ctx* ctx, const cafe_params* params, int32_t max_change, double level, const cafe_branch_change_out* out);
/* measurement: the summed HIP-event time in milliseconds of the band kernel's launches of the last cafe_branch_change when it
 * ran with profiling on (cafe_set_profiling), else 0 */
int cafe_debug_branch_change_band(cafe_ctx* ctx, double* ms);

/* Root rule of a context: what the scorer makes of a family's root vector L_j (j = 0..R-1 for root size j + 1).  A property of
 * the context, like the death rates: every later scoring call reads it.  CAFE_ROOT_MAX (the default) is the reference's rule,
 * max_j(L_j prior_j).  Under CAFE_ROOT_SUM a family's value is the marginal likelihood every posterior call conditions on:
 *   base model   family_lnl = log sum_j L_j prior_j, evaluated as m + log sum_j exp(t_j - m) with t_j = log L_j + log prior_j
 *                (the host's log of the float prior, as the max rule reads it) and m = max_j t_j: finite where the plain product
 *                underflows; all t_j = -inf gives -inf (the call's -lnL is then +inf); a NaN term gives NaN;
 *   gamma model  category_likelihood[f][k] = p_k sum_j L_j prior_j in the linear domain, family_likelihood their sum over k,
 *                family_lnl its log; failed[f] keeps the reference's rule (a category whose sum_j L_j is exactly 0).
 * The sum over j runs in a fixed order (16 interleaved row segments, combined in segment order): a value depends on the
 * family's column and R only, never on column chunks, graphs or the stream.  Honoured by cafe_score, cafe_score_partial /
 * cafe_finish_partial, cafe_family_results, cafe_score_per_family and cafe_score_per_family_lm; sharded use needs no entry of
 * its own: call the setter on every cafe_sharded_context(s, r).  It combines with death rates, error models, several lambdas
 * and several column chunks.  Not affected: cafe_root_max, cafe_pvalues, cafe_reconstruct, cafe_branch_probabilities (the
 * reference's own statistics) and every posterior call (each takes a root_rule or is defined on the sum).  With CAFE_ROOT_MAX
 * -- never set, or set back -- every result of every entry is bit for bit what it is without this setter.  Any other value:
 * CAFE_ERR_ARGUMENT, the rule stays. */
int cafe_set_root_rule(cafe_ctx* ctx, int32_t rule);
int cafe_get_root_rule(const cafe_ctx* ctx);      /* CAFE_ROOT_MAX or CAFE_ROOT_SUM; CAFE_ROOT_MAX for a NULL context */

/* Root posterior on the scorer's own prune: P(root size = j + 1 | data_f) for every family, summarised per family and summed
 * over the table -- the E step of a maximum-likelihood update of the root distribution, prior_new[j] = total[j] / n_used.  The
 * call runs the scorer's path (K1, the schedule with subtree sharing and zero extents, K2 / K3), not the sum-product engine,
 * and per column chunk two kernels stand where K4 does: one per column (Z, log Z, mean, mode, category posteriors and the
 * column's scale w_f / Z_f, w_f its multiplicity), one per root row (the weighted row sum of the panel).  The weights are
 * always the sum rule's, whatever cafe_set_root_rule says: with the gamma model
 * P(root = j + 1 | data) = sum_k p_k prior_j L^k_j / Z, Z = sum_k p_k sum_j prior_j L^k_j.  Outputs (host pointers, any may be
 * NULL), rows in the problem's family order:
 *   total[R] = sum over the families that did not fail of P(root size = j + 1 | data_f), every family of the table counted
 *     (identical families as often as they occur); n_used the number of those families, so sum_j total[j] = n_used to rounding.
 *     Per root row the 128-column tiles are folded in tile order, each tile summed by a fixed tree: total does not depend on
 *     workspace_limit, not even in the last bit;
 *   mean[n_families], mode[n_families] (first arg max, as a size 1..R) of the family's root posterior;
 *   category_posterior[n_families][K] = p_k Z_k / Z, gamma model only (CAFE_ERR_ARGUMENT otherwise);
 *   log_evidence[n_families] = log Z (base model: the log-sum-exp of cafe_set_root_rule, the bits cafe_score returns per
 *     family under CAFE_ROOT_SUM; gamma model likewise);
 *   failed[n_families] = 1 where Z is 0 or not finite: that family's doubles are NaN, its mode -1, and it adds nothing to total
 *     (the call still returns CAFE_OK).
 * Reads model, lambdas, n_categories, multipliers, cat_probs, prior and error_model of params; the context's death rates
 * apply.  CAFE_ERR_ARGUMENT for invalid rates or a bad K; CAFE_ERR_STATE on a context with a communicator attached.
 * cafe_family_results is not meaningful after this call; a later cafe_score is unaffected. */
typedef struct cafe_root_posterior_out {
    double*  total;              /* [R] */
    int64_t* n_used;             /* families that entered total */
    double*  mean;               /* [n_families] posterior mean root size */
    int32_t* mode;               /* [n_families] first arg max, as a size (1..R) */
    double*  category_posterior; /* [n_families][K]; gamma model only */
    double*  log_evidence;       /* [n_families] */
    int32_t* failed;             /* [n_families] */
} cafe_root_posterior_out;
int cafe_root_posterior(cafe_ctx* ctx, const cafe_params* params, const cafe_root_posterior_out* out);

/* Introspection for parity tests: the transition matrix the last call built for the branch above
 * `node` in category k (N x N row-major, N = max(M,R)+1: matrix_cache::get_matrix; for an interior
 * branch the columns c > M, which the prune never reads, are not materialised and come back 0), and the root
 * likelihood vector (R values: inference_prune's return) of family f in category k. */
int cafe_get_matrix(cafe_ctx* ctx, int32_t node, int32_t category, double* out, size_t out_len);
int cafe_get_root_likelihoods(cafe_ctx* ctx, int64_t family, int32_t category, double* out, size_t out_len);
/* The zero extents the last call worked with (parity tests: they must contain every non-zero).
 *   matrix_ext: the branch above `node` in `category` -- an interior branch: per block of 16 parent sizes s = 16b+1..16b+16
 *               the first / last child size with a non-zero entry, [ceil((N-1)/16)][2]; a leaf branch: per child size
 *               (column) x the first / last parent size with P[s][x] != 0, [N][2].  first > last: all zero.
 *   panel_ext:  interior non-root nodes, or NULL: per 128-column tile of the node's panel the first / last row (size) that
 *               may be non-zero, [columns / 128][2]; *n_tiles receives the number of tiles. */
int cafe_get_extents(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* matrix_ext, size_t matrix_ext_len,
                     int32_t* panel_ext, size_t panel_ext_len, int32_t* n_tiles);
/* diagnostic: the per-COLUMN zero extents of an interior non-root node's panel in the last call, out[columns][2] (rows outside
 * [lo, hi] of a column are exactly zero; lo > hi: the whole column); *n_cols receives the panel's (padded) column count */
int cafe_debug_column_extents(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* out, size_t out_len, int64_t* n_cols);
/* diagnostic: the magnitude bounds of an interior non-root node's panel in the last call (extents.hip, node_level_kernel):
 * out[tile * *row_steps + r] is an upper bound of log2 of every COMPUTED entry of panel rows 4 r .. 4 r + 3 in 128-column tile
 * `tile`, -inf where they are all exactly zero, never below -1060 otherwise.  out == NULL: the two sizes only.  CAFE_ERR_STATE
 * when the last call kept none (CAFE_NO_MAGSKIP, CAFE_NO_KSKIP, matrix order below 256, an error model). */
int cafe_debug_panel_bounds(cafe_ctx* ctx, int32_t node, int32_t category, double* out, size_t out_len, int32_t* n_tiles, int32_t* row_steps);
/* diagnostic: the narrowed hulls of an interior non-root node's panel in the last call, out[tile][2], laid out like
 * cafe_get_extents' panel_ext: the structural hull of a 128-column tile cut back from both ends over the steps of 4 rows whose
 * magnitude bound, before its floor, lies below 2^-1100 -- rows that hold computed zeros only, that the assemble passes do not
 * write and that no K range reaches (lo > hi: the whole tile).  Equal to panel_ext where the last call kept no bounds (the
 * state errors of cafe_debug_panel_bounds do not apply) and under CAFE_NO_NARROW=1.  *n_tiles receives the number of tiles. */
int cafe_debug_narrowed_extents(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* out, size_t out_len, int32_t* n_tiles);
/* diagnostic: one slot of the magnitude tables of the last call's matrices (extents.hip, mag_tables_kernel), as written: upper
 * bounds of log2 in units of 1/256, -(1 << 28) where every entry the item stands for is exactly zero.
 *   which 0: a16, out[ks * *n1 + b]  the largest P[s][c], s in 16 b + 1 .. 16 b + 16, c in 4 ks .. 4 ks + 3   (interior branch)
 *   which 1: t4,  out[ks * *n1 + r]  the largest sum of P[s][c] over those four c, s in 4 r .. 4 r + 3         (interior branch)
 *   which 2: lt,  out[x * *n1 + r]   the largest P[s][x], s in 4 r .. 4 r + 3, x = 0 .. M                      (leaf branch)
 * slot >= 0 names the matrix by its slot in the k-major (which 0, 1) or row-major (which 2) pool; slot < 0: the matrix of the
 * branch above `node` in `category`.  out == NULL: the two sizes only.  Never called on the scorer path.  The state errors are
 * those of cafe_debug_panel_bounds. */
int cafe_debug_magnitude_tables(cafe_ctx* ctx, int32_t which, int32_t slot, int32_t* out, size_t out_len, int32_t* n0, int32_t* n1,
                                int32_t node, int32_t category);
/* diagnostic: column tiles a workgroup of the per-level interval / bound kernel owns in the following calls (1, 2 or 4;
 * 0 = chosen per level from the level's size, the default).  No result, bound or range depends on it; calls made while
 * it is set are enqueued launch by launch (no graph replay). */
int cafe_debug_level_tiles(cafe_ctx* ctx, int tiles);
/* diagnostic: the K ranges of the K2 op that multiplies the matrix of the branch above `node` (interior, not the root) in the
 * last call: out[(tile * *n_blocks + b) * 2 + {0, 1}] = first / last k-step (4 deep) that 16-row block b of the matrix runs
 * against column tile `tile` of the node's panel (first > last: none).  The block's non-zero extent cut by the panel's and,
 * unless CAFE_NO_MAGSKIP is set, by the k-steps whose products all lie below 2^-1100.  out == NULL: the two sizes only. */
int cafe_debug_k_ranges(cafe_ctx* ctx, int32_t node, int32_t category, int32_t* out, size_t out_len, int32_t* n_tiles, int32_t* n_blocks);
/* diagnostic: leaf branches whose matrix the context keeps a transposed copy of (leaf_reduce.hip, leaf_transpose_kernel: a
 * leaf that meets an interior sibling's factor in an assemble pass), and whether the last call used the copies (it does not
 * when it carries an error model) */
int cafe_debug_leaf_transposes(cafe_ctx* ctx, int32_t* n_branches, int32_t* used_by_last_call);
int cafe_get_stats(const cafe_ctx* ctx, cafe_stats* stats);
/* Flops the K2 launches of the last call executed: a (row tile, column tile) pair runs only the K tiles inside the
 * intersection of the matrix's non-zero extent (K1) and the panel's (extents.hip), and of those each 16-row block of the tile
 * only the ones inside its own extent -- the products left out all have an exact zero in them.  Reads the extents back and counts on the host (milliseconds): measurement only.  Needs a call that
 * was enqueued launch by launch (no graph replay). */
int cafe_executed_flops(cafe_ctx* ctx, double* flops);
/* Flops of the MFMAs the K2 launches of the last call ISSUED.  cafe_executed_flops counts the products that have no exact
 * zero in them -- what the kernel issues under CAFE_NO_MAGSKIP=1.  By default a row block's K range is shorter still by the
 * k-steps at its ends whose products all lie below half the smallest denormal (cafe_debug_k_ranges): the same result bits,
 * fewer MFMAs, and this is their count (<= cafe_executed_flops, equal under CAFE_NO_MAGSKIP=1 or with an error model).  Over
 * a launch's time it is the rate of the matrix pipe; cafe_executed_flops over the same time is the rate at which the
 * non-zero products are dealt with, which may exceed the pipe's peak.  Same conditions as cafe_executed_flops. */
int cafe_issued_flops(cafe_ctx* ctx, double* flops);
/* diagnostic: the same count with every 16-row block of a tile taken over the tile's WHOLE K range (the hull of its blocks'
 * ranges) -- what the kernel issued until each block got its own range (prune_gemm.hip, block_ranges), and what rounds 2 and
 * 3a quoted their roofline fractions on; >= cafe_executed_flops */
int cafe_debug_tile_range_flops(cafe_ctx* ctx, double* flops);
/* diagnostic: the same per K2 launch of the last call, in launch order (executed[n], all_k_tiles[n] and tile_height[n] may be
 * NULL); n = cafe_stats.gemm_launches */
int cafe_debug_launch_flops(cafe_ctx* ctx, double* executed, double* all_k_tiles, int32_t* tile_height, size_t n);
int cafe_debug_launch_ms(cafe_ctx* ctx, double* ms, size_t n);      /* HIP-event duration of each (profiling on) */
/* diagnostic / test: reads back the tile lists the planner (extents.hip, tile_plan_kernel) laid out for the K2 launches of the
 * last call and checks that every tile appears exactly once with the K range its extents give; *n_planned = launches that ran
 * from a list, *worst_load = largest modelled workgroup load / mean load of its XCD.  CAFE_ERR_STATE on a mismatch. */
int cafe_debug_plan_check(cafe_ctx* ctx, int32_t* n_planned, double* worst_load);
int cafe_matrix_size(const cafe_ctx* ctx);
/* 1: bracket the phases and every K2 launch with HIP events so that cafe_stats.ms_* are measured (bench.py does).
 * 0 (default): no events. */
int cafe_set_profiling(cafe_ctx* ctx, int on);
/* 1: capture the call's fixed launch sequence once per (model, K) in a hipGraph and replay it (not while profiling);
 * 0 (default): enqueue launch by launch.  Same kernels, same
 * arguments, same bits; which is faster depends on the runtime. */
int cafe_set_graphs(cafe_ctx* ctx, int on);
/* diagnostic: K2's row tile is 16*mi rows, mi = 2..9, normally chosen per launch; mi forces one, 0 restores the choice */
int cafe_debug_force_tile(cafe_ctx* ctx, int mi);
/* test hook: the n-th next call of this context (n >= 1; 0 disarms) fails with CAFE_ERR_DEVICE behind its K1 launch, as a
 * HIP error in the middle of a call would -- pins the fail-together behaviour above */
int cafe_debug_fail_next(cafe_ctx* ctx, int n);
/* diagnostic (CAFE_GEMM_STAMPS=1 at cafe_create): per-block placement + timeline words of the last K2 launch */
int cafe_debug_stamps(cafe_ctx* ctx, unsigned long long* out, size_t words);
/* test hook: one cafe_pvalues call -- the same arguments, the same launches, the same p-values, bit for bit -- that also copies
 * what its stages left on the device into the caller's host arrays (any of them may be NULL), Fs = R * n_simulations, family
 * f = s * n_simulations + i simulated from root size s:
 *   sizes[n_nodes][Fs]        the simulated size of every node (simulate_kernel's scratch);
 *   counts[n_taxa][Fs]        the leaf counts as the context of the simulated families reads them: its taxon-major table, read
 *                             with its own leading dimension and cut to Fs columns;
 *   cond_unsorted[R][n_simulations], cond_sorted[R][n_simulations]
 *                             that context's root maxima before and after sort_rows_kernel;
 *   observed[n_families]      the observed families' root maxima the p-value kernel read, spread to the listed families.
 * The copies cost synchronous transfers and two waits that cafe_pvalues does not make: for tests, not for timing. */
typedef struct cafe_pvalue_stages {
    int32_t* sizes;
    int32_t* counts;
    double*  cond_unsorted;
    double*  cond_sorted;
    double*  observed;
} cafe_pvalue_stages;
int cafe_debug_pvalues_stages(cafe_ctx* ctx, const cafe_params* params, int32_t n_simulations, uint64_t seed,
                              const cafe_pvalue_stages* stages, double* pvalues);

/* Stand-alone kernels exposed for unit parity tests and the roofline probe. */
/* builds `count` matrices of order n for (lambda[i], t[i]) pairs with matrix_cache_key quantization
 * applied (matrix_cache.h:42-61); out[count][n][n] is always P[s][c] row-major.  layout 0: the row-major
 * device layout leaf branches use; layout 1: the k-major layout of interior branches (built through the
 * reversibility relation, see bd_matrix.hip), converted back on the host. */
int cafe_build_matrices(int32_t device, int32_t n, int32_t count, const double* lambdas, const double* ts, int32_t layout, double* out);
/* the same under separate birth and death rates (lambdas[i], mus[i], ts[i]): K1's two-rate instantiation (bd_matrix_lm.hip) */
int cafe_build_matrices_lm(int32_t device, int32_t n, int32_t count, const double* lambdas, const double* mus, const double* ts,
                           int32_t layout, double* out);
/* cafe_pvalues' two closing kernels alone, on host arrays, launched as cafe_pvalues launches them (pvalues.hip):
 *   cafe_debug_sort_rows    sorts each of the `rows` rows of values[rows][n] ascending in place (sort_rows_kernel, one block
 *                           per row, n = 1..2048);
 *   cafe_debug_tree_pvalue  pvalues[f] = max over the n_root_sizes rows of cond[n_root_sizes][n] (each sorted ascending) of
 *                           the number of entries <= observed[f], a count of n reported as n - 1, over n (tree_pvalue_kernel).
 * CAFE_ERR_ARGUMENT for a NULL array or a size outside those ranges. */
int cafe_debug_sort_rows(int32_t device, double* values, int32_t rows, int32_t n);
int cafe_debug_tree_pvalue(int32_t device, const double* observed, int64_t n_observed, const double* cond, int32_t n_root_sizes,
                           int32_t n, double* pvalues);
/* The weighted Gram matrix of cafe_branch_scores alone: gram[p][p] = S diag(w) S^T and total[p] = S w for S [p][n] row-major,
 * host pointers (gram or total may be NULL).  One wave forms one 16 x 16 tile of the lower triangle over one slab of 2048
 * columns on v_mfma_f64_16x16x4_f64; the slabs' partial tiles are added in slab order and the upper triangle is the mirror
 * image, so gram is exactly symmetric and its bits depend on (p, n) alone.  A column of weight 0 adds exactly 0 whatever it
 * holds. */
int cafe_weighted_gram(int32_t device, int32_t p, int64_t n, const double* S, const double* w, double* gram, double* total);
/* back-to-back v_mfma_f64_16x16x4_f64 issue-rate probe: returns achieved TFLOP/s on `device`. */
int cafe_probe_fp64_mfma(int32_t device, double* tflops);

#ifdef __cplusplus
}
#endif
#endif
