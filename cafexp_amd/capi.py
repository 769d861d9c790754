"""ctypes binding of libcafe_mi355x.so (the C ABI declared in include/cafe_mi355x.h).

Plumbing only: builds the C structs from `problem.Problem` / `problem.Params`, calls the library
and raises on error codes.  There is no fallback: if the HIP library is missing or no GPU is
usable, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .problem import Params, Problem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcafe_mi355x.so")

CAFE_MAX_CATEGORIES = 32
CAFE_FLAG_NO_DEDUP = 1
CAFE_FLAG_NO_SUBTREE_DEDUP = 2
CAFE_FLAG_MISSING_COUNTS = 4     # counts may hold CAFE_COUNT_MISSING (Problem.missing_counts sets it)
CAFE_COUNT_MISSING = -1
CAFE_FAMILY_ABSENT = -1          # cafe_score_per_family_gain: the profile with every count 0, whether or not the table holds it
CAFE_MODEL_BASE, CAFE_MODEL_GAMMA = 0, 1
CAFE_ROOT_MAX, CAFE_ROOT_SUM = 0, 1

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_f32p = C.POINTER(C.c_float)


class CafeProblem(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int32), ("parent", _i32p), ("branch_length", _f64p), ("lambda_index", _i32p),
        ("leaf_taxon", _i32p), ("n_taxa", C.c_int32), ("n_families", C.c_int64), ("counts", _i32p),
        ("max_family_size", C.c_int32), ("max_root_family_size", C.c_int32), ("n_lambdas", C.c_int32),
        ("single_lambda", C.c_int32), ("max_categories", C.c_int32), ("n_deviations", C.c_int32),
        ("device", C.c_int32), ("flags", C.c_int32), ("workspace_limit", C.c_size_t),
    ]


class CafeParams(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("lambdas", _f64p), ("n_categories", C.c_int32), ("multipliers", _f64p),
        ("cat_probs", _f64p), ("alpha", C.c_double), ("prior", _f32p), ("error_model", _f64p),
    ]


class CafeBatchParams(C.Structure):
    _fields_ = [
        ("n_points", C.c_int32), ("model", C.c_int32), ("n_categories", C.c_int32), ("lambdas", _f64p), ("mus", _f64p),
        ("multipliers", _f64p), ("cat_probs", _f64p), ("alpha", _f64p), ("prior", _f32p), ("error_model", _f64p),
    ]


class CafeFamilyOut(C.Structure):
    _fields_ = [("family_lnl", _f64p), ("category_likelihood", _f64p), ("family_likelihood", _f64p), ("failed", _i32p)]


class CafeMarginalOut(C.Structure):
    _fields_ = [("mean", _f64p), ("mode", _i32p), ("lo", _i32p), ("hi", _i32p), ("p_increase", _f64p), ("p_decrease", _f64p),
                ("log_evidence", _f64p), ("failed", _i32p)]


class CafeGradientOut(C.Structure):
    _fields_ = [("family_lnl", _f64p), ("d_lambda", _f64p), ("d_mu", _f64p), ("d_multiplier", _f64p), ("failed", _i32p)]


class CafeBranchScoresOut(C.Structure):
    _fields_ = [("rate", _f64p), ("birth", _f64p), ("death", _f64p), ("family_lnl", _f64p), ("d_lambda", _f64p), ("d_mu", _f64p),
                ("d_multiplier", _f64p), ("failed", _i32p), ("total", _f64p), ("gram", _f64p), ("n_used", _i64p)]


class CafeEventsOut(C.Structure):
    _fields_ = [("gains", _f64p), ("losses", _f64p), ("log_evidence", _f64p), ("failed", _i32p)]


class CafeGainPosteriorOut(C.Structure):
    _fields_ = [("lnl", _f64p), ("p_absent", _f64p), ("mean", _f64p), ("p_gain", _f64p), ("p_loss", _f64p), ("posterior", _f64p)]


class CafeLeafPredictiveOut(C.Structure):
    _fields_ = [("mean", _f64p), ("sd", _f64p), ("p_below", _f64p), ("p_obs", _f64p), ("p_above", _f64p), ("log_evidence", _f64p),
                ("failed", _i32p)]


class CafeBranchChangeOut(C.Structure):
    _fields_ = [("pmf", _f64p), ("below", _f64p), ("above", _f64p), ("mean", _f64p), ("mode", _i32p), ("lo", _i32p), ("hi", _i32p),
                ("log_evidence", _f64p), ("failed", _i32p)]


class CafeRootPosteriorOut(C.Structure):
    _fields_ = [("total", _f64p), ("n_used", _i64p), ("mean", _f64p), ("mode", _i32p), ("category_posterior", _f64p),
                ("log_evidence", _f64p), ("failed", _i32p)]


class CafeHistoryOut(C.Structure):
    _fields_ = [("sizes", _i32p), ("category", _i32p), ("n_increase", _i64p), ("n_decrease", _i64p), ("net_change", _i64p),
                ("log_evidence", _f64p), ("failed", _i32p)]


class CafePvalueStages(C.Structure):
    _fields_ = [("sizes", _i32p), ("counts", _i32p), ("cond_unsorted", _f64p), ("cond_sorted", _f64p), ("observed", _f64p)]


class CafeStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_double), ("ms_matrices", C.c_double), ("ms_prune", C.c_double), ("ms_gemm", C.c_double),
        ("ms_reduce", C.c_double), ("gemm_flops", C.c_double), ("gemm_bytes", C.c_double), ("gemm_flops_per_family", C.c_double),
        ("gemm_launches", C.c_int64), ("n_matrices", C.c_int64), ("n_unique_families", C.c_int64),
        ("n_chunks", C.c_int64), ("matrix_bytes", C.c_int64), ("panel_bytes", C.c_int64),
        ("n_assemble_passes", C.c_int64), ("n_gather_epilogues", C.c_int64), ("n_leaf_passes", C.c_int64),
        ("gemm_flops_dense", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CafeSimProblem(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int32), ("parent", _i32p), ("branch_length", _f64p), ("lambda_index", _i32p), ("leaf_taxon", _i32p),
        ("n_taxa", C.c_int32), ("n_lambdas", C.c_int32), ("lambdas", _f64p), ("max_family_size", C.c_int32),
        ("n_families", C.c_int64), ("root_size", _i32p), ("chunk_size", C.c_int32), ("chunk_multiplier", _f64p),
        ("n_deviations", C.c_int32), ("error_model", _f64p), ("error_model_max_size", C.c_int32), ("device", C.c_int32),
        ("workspace_limit", C.c_size_t),
    ]


EXPORTS = [
    "cafe_abi_version", "cafe_create", "cafe_destroy", "cafe_last_error", "cafe_score", "cafe_score_partial",
    "cafe_finish_partial", "cafe_family_results", "cafe_get_matrix", "cafe_get_root_likelihoods", "cafe_get_stats",
    "cafe_matrix_size", "cafe_build_matrices", "cafe_probe_fp64_mfma", "cafe_set_profiling", "cafe_debug_stamps",
    "cafe_root_max", "cafe_reconstruct", "cafe_branch_probabilities", "cafe_pvalues", "cafe_debug_force_tile",
    "cafe_comm_unique_id", "cafe_comm_attach", "cafe_comm_detach", "cafe_shard_plan", "cafe_shard_plan_scaled", "cafe_create_sharded",
    "cafe_sharded_destroy", "cafe_sharded_last_error", "cafe_sharded_score", "cafe_sharded_family_results",
    "cafe_sharded_size", "cafe_sharded_context", "cafe_set_graphs", "cafe_executed_flops", "cafe_debug_tile_range_flops", "cafe_get_extents", "cafe_debug_launch_flops", "cafe_debug_launch_ms", "cafe_debug_plan_check",
    "cafe_debug_fail_next", "cafe_debug_column_extents", "cafe_debug_panel_bounds", "cafe_debug_k_ranges", "cafe_issued_flops", "cafe_debug_leaf_transposes", "cafe_simulate",
    "cafe_score_per_family", "cafe_marginal_reconstruct", "cafe_debug_marginal_gemm", "cafe_sample_histories", "cafe_debug_history_batches",
    "cafe_set_death_rates", "cafe_bd_rates", "cafe_build_matrices_lm", "cafe_score_per_family_lm", "cafe_simulate_lm",
    "cafe_score_gradient", "cafe_bd_rates_grad", "cafe_expected_events", "cafe_bd_rates_events",
    "cafe_branch_scores", "cafe_branch_scores_dim", "cafe_weighted_gram", "cafe_debug_gram",
    "cafe_leaf_predictive", "cafe_set_root_rule", "cafe_get_root_rule", "cafe_root_posterior", "cafe_debug_magnitude_tables", "cafe_debug_level_tiles",
    "cafe_branch_change", "cafe_debug_branch_change_band", "cafe_score_batch",
    "cafe_score_per_family_gain", "cafe_bd_gain_row0", "cafe_debug_narrowed_extents", "cafe_gain_posterior",
    "cafe_debug_pvalues_stages", "cafe_debug_sort_rows", "cafe_debug_tree_pvalue",
]
CAFE_CHANGE_NONE = -(1 << 31)   # mode / lo / hi of cafe_branch_change at the root and in a failed family
CAFE_COMM_ID_BYTES = 128
MAG_NONE = -(1 << 28)           # a magnitude-table entry whose items are all exactly zero (cafe_kernels.h, kMagNone)
MAG_UNIT = 256                  # table units per power of two

_lib = None


class CafeError(RuntimeError):
    pass


def load():
    """dlopen the HIP library; raises CafeError when it was not built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own libamdhip64.so.7; two HIP runtimes in one process cannot both own
    # the GPU.  Importing torch first makes this library bind to the runtime torch already loaded
    # (same SONAME), so torch tensors / streams / torch.distributed (RCCL) and these kernels share it.
    if os.environ.get("CAFE_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise CafeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.cafe_abi_version.restype = C.c_int
    L.cafe_create.restype = C.c_void_p
    L.cafe_create.argtypes = [C.POINTER(CafeProblem), C.c_char_p, C.c_size_t]
    L.cafe_destroy.argtypes = [C.c_void_p]
    L.cafe_destroy.restype = None
    L.cafe_last_error.restype = C.c_char_p
    L.cafe_last_error.argtypes = [C.c_void_p]
    L.cafe_score.restype = C.c_int
    L.cafe_score.argtypes = [C.c_void_p, C.POINTER(CafeParams), _f64p, C.POINTER(CafeFamilyOut)]
    L.cafe_score_batch.restype = C.c_int
    L.cafe_score_batch.argtypes = [C.c_void_p, C.POINTER(CafeBatchParams), _f64p]
    L.cafe_score_partial.restype = C.c_int
    L.cafe_score_partial.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_void_p, C.c_void_p]
    L.cafe_finish_partial.restype = C.c_double
    L.cafe_finish_partial.argtypes = [_f64p]
    L.cafe_family_results.restype = C.c_int
    L.cafe_family_results.argtypes = [C.c_void_p, C.POINTER(CafeFamilyOut)]
    L.cafe_get_matrix.restype = C.c_int
    L.cafe_get_matrix.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _f64p, C.c_size_t]
    L.cafe_get_root_likelihoods.restype = C.c_int
    L.cafe_get_root_likelihoods.argtypes = [C.c_void_p, C.c_int64, C.c_int32, _f64p, C.c_size_t]
    L.cafe_root_max.restype = C.c_int
    L.cafe_root_max.argtypes = [C.c_void_p, C.POINTER(CafeParams), _f64p]
    L.cafe_score_per_family.restype = C.c_int
    L.cafe_score_per_family.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int64, _i64p, _f64p, _f64p]
    L.cafe_score_per_family_lm.restype = C.c_int
    L.cafe_score_per_family_lm.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int64, _i64p, _f64p, _f64p, _f64p]
    L.cafe_marginal_reconstruct.restype = C.c_int
    L.cafe_marginal_reconstruct.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_double, C.POINTER(CafeMarginalOut)]
    L.cafe_sample_histories.restype = C.c_int
    L.cafe_sample_histories.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int32, C.c_uint64, C.POINTER(CafeHistoryOut)]
    L.cafe_debug_marginal_gemm.restype = C.c_int
    L.cafe_debug_marginal_gemm.argtypes = [C.c_void_p, _f64p, _f64p]
    L.cafe_pvalues.restype = C.c_int
    L.cafe_pvalues.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int32, C.c_uint64, _f64p]
    L.cafe_reconstruct.restype = C.c_int
    L.cafe_reconstruct.argtypes = [C.c_void_p, C.POINTER(CafeParams), _f32p, _i32p]
    L.cafe_branch_probabilities.restype = C.c_int
    L.cafe_branch_probabilities.argtypes = [C.c_void_p, C.POINTER(CafeParams), _i32p, _f64p]
    L.cafe_get_stats.restype = C.c_int
    L.cafe_get_stats.argtypes = [C.c_void_p, C.POINTER(CafeStats)]
    L.cafe_matrix_size.restype = C.c_int
    L.cafe_matrix_size.argtypes = [C.c_void_p]
    L.cafe_build_matrices.restype = C.c_int
    L.cafe_build_matrices.argtypes = [C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p, C.c_int32, _f64p]
    L.cafe_build_matrices_lm.restype = C.c_int
    L.cafe_build_matrices_lm.argtypes = [C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p, _f64p, C.c_int32, _f64p]
    L.cafe_set_death_rates.restype = C.c_int
    L.cafe_set_death_rates.argtypes = [C.c_void_p, _f64p]
    L.cafe_score_per_family_gain.restype = C.c_int
    L.cafe_score_per_family_gain.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int64, _i64p, _f64p, _f64p, _f64p, C.c_double, _f64p]
    L.cafe_gain_posterior.restype = C.c_int
    L.cafe_gain_posterior.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int64, _i64p, _f64p, _f64p, _f64p, C.c_double,
                                      C.POINTER(CafeGainPosteriorOut)]
    L.cafe_bd_gain_row0.restype = C.c_int
    L.cafe_bd_gain_row0.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, _f64p, _f64p]
    L.cafe_bd_rates.restype = C.c_int
    L.cafe_bd_rates.argtypes = [C.c_double, C.c_double, C.c_double, _f64p]
    L.cafe_score_gradient.restype = C.c_int
    L.cafe_score_gradient.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int32, C.POINTER(CafeGradientOut)]
    L.cafe_bd_rates_grad.restype = C.c_int
    L.cafe_bd_rates_grad.argtypes = [C.c_double, C.c_double, C.c_double, _f64p]
    L.cafe_expected_events.restype = C.c_int
    L.cafe_expected_events.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.POINTER(CafeEventsOut)]
    L.cafe_bd_rates_events.restype = C.c_int
    L.cafe_bd_rates_events.argtypes = [C.c_double, C.c_double, C.c_double, _f64p]
    L.cafe_leaf_predictive.restype = C.c_int
    L.cafe_leaf_predictive.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.POINTER(CafeLeafPredictiveOut)]
    L.cafe_branch_change.restype = C.c_int
    L.cafe_branch_change.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int32, C.c_double, C.POINTER(CafeBranchChangeOut)]
    L.cafe_debug_branch_change_band.restype = C.c_int
    L.cafe_debug_branch_change_band.argtypes = [C.c_void_p, _f64p]
    L.cafe_set_root_rule.restype = C.c_int
    L.cafe_set_root_rule.argtypes = [C.c_void_p, C.c_int32]
    L.cafe_get_root_rule.restype = C.c_int
    L.cafe_get_root_rule.argtypes = [C.c_void_p]
    L.cafe_root_posterior.restype = C.c_int
    L.cafe_root_posterior.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.POINTER(CafeRootPosteriorOut)]
    L.cafe_branch_scores.restype = C.c_int
    L.cafe_branch_scores.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int32, C.POINTER(CafeBranchScoresOut)]
    L.cafe_branch_scores_dim.restype = C.c_int
    L.cafe_branch_scores_dim.argtypes = [C.c_void_p, C.POINTER(CafeParams), _i32p]
    L.cafe_debug_gram.restype = C.c_int
    L.cafe_debug_gram.argtypes = [C.c_void_p, _f64p, _f64p]
    L.cafe_weighted_gram.restype = C.c_int
    L.cafe_weighted_gram.argtypes = [C.c_int32, C.c_int32, C.c_int64, _f64p, _f64p, _f64p, _f64p]
    L.cafe_probe_fp64_mfma.restype = C.c_int
    L.cafe_probe_fp64_mfma.argtypes = [C.c_int32, _f64p]
    L.cafe_debug_stamps.restype = C.c_int
    L.cafe_debug_stamps.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]
    L.cafe_debug_force_tile.restype = C.c_int
    L.cafe_debug_force_tile.argtypes = [C.c_void_p, C.c_int]
    L.cafe_set_profiling.restype = C.c_int
    L.cafe_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.cafe_set_graphs.restype = C.c_int
    L.cafe_set_graphs.argtypes = [C.c_void_p, C.c_int]
    L.cafe_get_extents.restype = C.c_int
    L.cafe_get_extents.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _i32p, C.c_size_t, _i32p, C.c_size_t, _i32p]
    L.cafe_debug_launch_flops.restype = C.c_int
    L.cafe_debug_launch_flops.argtypes = [C.c_void_p, _f64p, _f64p, _i32p, C.c_size_t]
    L.cafe_executed_flops.restype = C.c_int
    L.cafe_executed_flops.argtypes = [C.c_void_p, _f64p]
    L.cafe_comm_unique_id.restype = C.c_int
    L.cafe_comm_unique_id.argtypes = [C.c_char_p]
    L.cafe_comm_attach.restype = C.c_int
    L.cafe_comm_attach.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]
    L.cafe_comm_detach.restype = C.c_int
    L.cafe_comm_detach.argtypes = [C.c_void_p]
    L.cafe_shard_plan.restype = C.c_int
    L.cafe_shard_plan.argtypes = [C.POINTER(CafeProblem), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.cafe_create_sharded.restype = C.c_void_p
    L.cafe_create_sharded.argtypes = [C.POINTER(CafeProblem), _i32p, C.c_int32, C.c_char_p, C.c_size_t]
    L.cafe_sharded_destroy.restype = None
    L.cafe_sharded_destroy.argtypes = [C.c_void_p]
    L.cafe_sharded_last_error.restype = C.c_char_p
    L.cafe_sharded_last_error.argtypes = [C.c_void_p]
    L.cafe_sharded_score.restype = C.c_int
    L.cafe_sharded_score.argtypes = [C.c_void_p, C.POINTER(CafeParams), _f64p, C.POINTER(CafeFamilyOut)]
    L.cafe_sharded_family_results.restype = C.c_int
    L.cafe_sharded_family_results.argtypes = [C.c_void_p, C.POINTER(CafeFamilyOut)]
    L.cafe_sharded_size.restype = C.c_int32
    L.cafe_sharded_size.argtypes = [C.c_void_p]
    L.cafe_sharded_context.restype = C.c_void_p
    L.cafe_sharded_context.argtypes = [C.c_void_p, C.c_int32]
    L.cafe_debug_fail_next.restype = C.c_int
    L.cafe_debug_fail_next.argtypes = [C.c_void_p, C.c_int]
    L.cafe_simulate.restype = C.c_int
    L.cafe_simulate.argtypes = [C.POINTER(CafeSimProblem), C.c_uint64, _i32p, _i32p, C.c_char_p, C.c_size_t]
    L.cafe_simulate_lm.restype = C.c_int
    L.cafe_simulate_lm.argtypes = [C.POINTER(CafeSimProblem), _f64p, C.c_uint64, _i32p, _i32p, C.c_char_p, C.c_size_t]
    _lib = L
    return L


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def _c_problem(pb: Problem, keep: list, max_categories: int = 1, device: int = 0, flags: int = 0, workspace_limit: int = 0) -> CafeProblem:
    def k(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a
    cp = CafeProblem()
    cp.n_nodes = pb.n_nodes
    cp.parent = _p(k(pb.parent, np.int32), _i32p)
    cp.branch_length = _p(k(pb.branch_length, np.float64), _f64p)
    cp.lambda_index = _p(k(pb.lambda_index, np.int32), _i32p)
    cp.leaf_taxon = _p(k(pb.leaf_taxon, np.int32), _i32p)
    cp.n_taxa = pb.n_taxa
    cp.n_families = pb.n_families
    cp.counts = _p(k(pb.counts, np.int32), _i32p)
    cp.max_family_size = pb.max_family_size
    cp.max_root_family_size = pb.max_root_family_size
    cp.n_lambdas = pb.n_lambdas
    cp.single_lambda = 1 if pb.single_lambda else 0
    cp.max_categories = max_categories
    cp.n_deviations = pb.n_deviations
    cp.device = device
    cp.flags = flags | (CAFE_FLAG_MISSING_COUNTS if getattr(pb, "missing_counts", False) else 0)
    cp.workspace_limit = workspace_limit
    return cp


def _c_params(pr: Params, alpha: float = 1.0):
    keep = []

    def k(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a
    cp = CafeParams()
    cp.model = CAFE_MODEL_GAMMA if pr.multipliers is not None else CAFE_MODEL_BASE
    cp.lambdas = _p(k(pr.lambdas, np.float64), _f64p)
    if pr.multipliers is not None:
        cp.n_categories = len(pr.multipliers)
        cp.multipliers = _p(k(pr.multipliers, np.float64), _f64p)
        cp.cat_probs = _p(k(pr.cat_probs, np.float64), _f64p) if pr.cat_probs is not None else None
    else:
        cp.n_categories = 1
    cp.alpha = alpha
    cp.prior = _p(k(pr.prior, np.float32), _f32p)
    cp.error_model = _p(k(pr.error_model, np.float64), _f64p) if pr.error_model is not None else None
    return cp, keep


def shard_plan(pb: Problem, n_shards: int, max_categories: int = 1, family_scale=None):
    """cafe_shard_plan / cafe_shard_plan_scaled: the library's balanced family partition (host code, no GPU needed).
    family_scale: per family (table order), measured time of its shard under an earlier plan / mean over that plan's shards.
    Returns the family indices of every shard (a list of n_shards int64 arrays)."""
    keep = []
    cp = _c_problem(pb, keep, max_categories)
    order = np.empty(pb.n_families, dtype=np.int64)
    bounds = np.empty(n_shards + 1, dtype=np.int64)
    L = load()
    if family_scale is None:
        rc = L.cafe_shard_plan(C.byref(cp), n_shards, order.ctypes.data_as(C.POINTER(C.c_int64)), bounds.ctypes.data_as(C.POINTER(C.c_int64)))
    else:
        fs = np.ascontiguousarray(family_scale, dtype=np.float64)
        assert fs.shape == (pb.n_families,)
        L.cafe_shard_plan_scaled.restype = C.c_int
        L.cafe_shard_plan_scaled.argtypes = [C.POINTER(CafeProblem), C.c_int32, _f64p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        rc = L.cafe_shard_plan_scaled(C.byref(cp), n_shards, _p(fs, _f64p), order.ctypes.data_as(C.POINTER(C.c_int64)), bounds.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc:
        raise CafeError("cafe_shard_plan failed with code %d" % rc)
    return [order[bounds[r]:bounds[r + 1]].copy() for r in range(n_shards)]


def rebalanced_plan(pb: Problem, plan, times, max_categories: int = 1, scale=None, return_scale: bool = False):
    """One step of measured rebalancing: `times[r]` is what shard r of `plan` took; the new plan (same number of shards) is
    made with every family scaled by its shard's time over the mean -- on top of `scale` (per family, table order) when
    `plan` itself came from an earlier step."""
    t = np.asarray(times, dtype=np.float64)
    scale = np.ones(pb.n_families) if scale is None else np.array(scale, dtype=np.float64)
    for r, fam in enumerate(plan):
        scale[fam] *= t[r] / t.mean()
    scale = np.clip(scale, 0.2, 5.0)
    new = shard_plan(pb, len(plan), max_categories, family_scale=scale)
    return (new, scale) if return_scale else new


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(CAFE_COMM_ID_BYTES)
    rc = load().cafe_comm_unique_id(buf)
    if rc:
        raise CafeError("cafe_comm_unique_id failed with code %d" % rc)
    return buf.raw


class Context:
    """One cafe_ctx: a family shard resident on one GPU (model state of the reference's scorer)."""

    def __init__(self, pb: Problem, max_categories: int = 1, device: int = 0, dedup: bool = True,
                 workspace_limit: int = 0, subtree_dedup: bool = True):
        self._lib = load()
        self._keep = []
        cp = _c_problem(pb, self._keep, max_categories, device,
                        (0 if dedup else CAFE_FLAG_NO_DEDUP) | (0 if subtree_dedup else CAFE_FLAG_NO_SUBTREE_DEDUP), workspace_limit)
        err = C.create_string_buffer(512)
        self._h = self._lib.cafe_create(C.byref(cp), err, 512)
        if not self._h:
            raise CafeError(err.value.decode() or "cafe_create failed")
        self.problem = pb
        self.R = pb.max_root_family_size
        self.M = pb.max_family_size
        self.n_nodes = pb.n_nodes
        self.n_families = pb.n_families
        self._keep = []          # cafe_create copied everything

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cafe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise CafeError("code %d: %s" % (rc, self._lib.cafe_last_error(self._h).decode()))

    def _params(self, pr: Params, alpha: float = 1.0):
        return _c_params(pr, alpha)

    def comm_attach(self, comm_id: bytes, world_size: int, rank: int):
        """Join the RCCL communicator of the ranks holding the other family shards: from now on score() all-reduces
        {sum lnL, rejects} and returns the whole table's value on every rank (collective call)."""
        self._check(self._lib.cafe_comm_attach(self._h, comm_id, world_size, rank))

    def comm_detach(self):
        self._check(self._lib.cafe_comm_detach(self._h))

    def score(self, pr: Params, alpha: float = 1.0, per_family: bool = False):
        """One infer_family_likelihoods call -> -lnL (float, may be inf / nan)."""
        cp, keep = self._params(pr, alpha)
        out = C.c_double()
        self._check(self._lib.cafe_score(self._h, C.byref(cp), C.byref(out), None))
        if not per_family:
            return out.value
        return out.value, self.family_results(len(pr.multipliers) if pr.multipliers is not None else 0)

    def score_batch(self, points, alphas=None, mus=None) -> np.ndarray:
        """cafe_score_batch: -lnL of several parameter vectors in one call, a float64 array with score()'s bits for each.
        points: Params of one model (all base, or all gamma with the same number of categories); prior and error model are the
        first point's, shared by the batch.  alphas: one per point (gamma; default 1.0).  mus: [len(points)][n_lambdas] death
        rates per point (the context must have death rates set), None: the context's own."""
        points = list(points)
        G = len(points)
        if G < 1:
            raise ValueError("score_batch needs at least one point")
        gamma = points[0].multipliers is not None
        K = len(points[0].multipliers) if gamma else 1
        for pr in points:
            if (pr.multipliers is not None) != gamma or (gamma and len(pr.multipliers) != K):
                raise ValueError("the points of a batch share one model and one number of categories")
        bp = CafeBatchParams()
        bp.n_points, bp.model, bp.n_categories = G, (CAFE_MODEL_GAMMA if gamma else CAFE_MODEL_BASE), K
        lam = np.ascontiguousarray([np.atleast_1d(pr.lambdas) for pr in points], dtype=np.float64)
        if lam.shape != (G, self.problem.n_lambdas):
            raise ValueError("every point needs %d lambdas" % self.problem.n_lambdas)
        bp.lambdas = _p(lam, _f64p)
        mu = None
        if mus is not None:
            mu = np.ascontiguousarray(mus, dtype=np.float64).reshape(G, -1)
            if mu.shape != lam.shape:
                raise ValueError("mus must be [%d][%d]" % lam.shape)
            bp.mus = _p(mu, _f64p)
        if gamma:
            mult = np.ascontiguousarray([pr.multipliers for pr in points], dtype=np.float64)
            cat = np.ascontiguousarray([pr.cat_probs for pr in points], dtype=np.float64)
            al = np.ascontiguousarray(np.ones(G) if alphas is None else alphas, dtype=np.float64)
            if mult.shape != (G, K) or cat.shape != (G, K) or al.shape != (G,):
                raise ValueError("multipliers and cat_probs must be [%d][%d], alphas [%d]" % (G, K, G))
            bp.multipliers, bp.cat_probs, bp.alpha = _p(mult, _f64p), _p(cat, _f64p), _p(al, _f64p)
        prior = np.ascontiguousarray(points[0].prior, dtype=np.float32)
        bp.prior = _p(prior, _f32p)
        err = np.ascontiguousarray(points[0].error_model, dtype=np.float64) if points[0].error_model is not None else None
        bp.error_model = _p(err, _f64p)
        out = np.empty(G)
        self._check(self._lib.cafe_score_batch(self._h, C.byref(bp), _p(out, _f64p)))
        return out

    def family_results(self, K: int = 0):
        F = self.n_families
        fo = CafeFamilyOut()
        res = {"family_lnl": np.empty(F), "failed": np.empty(F, dtype=np.int32)}
        fo.family_lnl = _p(res["family_lnl"], _f64p)
        fo.failed = _p(res["failed"], _i32p)
        if K > 0:
            res["category_likelihood"] = np.empty((F, K))
            res["family_likelihood"] = np.empty(F)
            fo.category_likelihood = _p(res["category_likelihood"], _f64p)
            fo.family_likelihood = _p(res["family_likelihood"], _f64p)
        self._check(self._lib.cafe_family_results(self._h, C.byref(fo)))
        return res

    def score_per_family(self, pr: Params, family, lambdas) -> np.ndarray:
        """cafe_score_per_family: lnL of every listed family under ITS OWN lambdas (lambdas[n][n_lambdas]; a 1-d array is
        one lambda per family).  -inf where score() would return +inf for that vector.  pr gives the prior and the error
        model; pr.lambdas is not read.  Base model only."""
        fam = np.ascontiguousarray(family, dtype=np.int64).reshape(-1)
        lam = np.ascontiguousarray(lambdas, dtype=np.float64).reshape(len(fam), -1)
        if lam.shape[1] != self.problem.n_lambdas:
            raise ValueError("lambdas must be [%d][%d]" % (len(fam), self.problem.n_lambdas))
        cp, keep = self._params(pr)
        out = np.empty(len(fam))
        self._check(self._lib.cafe_score_per_family(self._h, C.byref(cp), len(fam), _p(fam, _i64p), _p(lam, _f64p), _p(out, _f64p)))
        return out

    def score_per_family_lm(self, pr: Params, family, lambdas, mus) -> np.ndarray:
        """cafe_score_per_family_lm: lnL of every listed family under ITS OWN birth and death rates (lambdas and mus
        [n][n_lambdas]; 1-d arrays are one rate per family).  The context's death rates are not read.  Otherwise
        score_per_family."""
        fam = np.ascontiguousarray(family, dtype=np.int64).reshape(-1)
        lam = np.ascontiguousarray(lambdas, dtype=np.float64).reshape(len(fam), -1)
        mu = np.ascontiguousarray(mus, dtype=np.float64).reshape(len(fam), -1)
        if lam.shape[1] != self.problem.n_lambdas or mu.shape != lam.shape:
            raise ValueError("lambdas and mus must be [%d][%d]" % (len(fam), self.problem.n_lambdas))
        cp, keep = self._params(pr)
        out = np.empty(len(fam))
        self._check(self._lib.cafe_score_per_family_lm(self._h, C.byref(cp), len(fam), _p(fam, _i64p), _p(lam, _f64p), _p(mu, _f64p),
                                                       _p(out, _f64p)))
        return out

    def score_per_family_gain(self, pr: Params, family, lambdas, mus, nus, root_absent: float = 0.0) -> np.ndarray:
        """cafe_score_per_family_gain: lnL of every listed family under ITS OWN birth, death and gain rates (lambdas, mus and
        nus [n][n_lambdas]; 1-d arrays are one rate per family; mus None: mu = lambda), root sizes 0..R with mass root_absent
        at 0.  family may hold CAFE_FAMILY_ABSENT, the all-zero profile.  Otherwise score_per_family_lm."""
        fam = np.ascontiguousarray(family, dtype=np.int64).reshape(-1)
        lam = np.ascontiguousarray(lambdas, dtype=np.float64).reshape(len(fam), -1)
        nu = np.ascontiguousarray(nus, dtype=np.float64).reshape(len(fam), -1)
        mu = None if mus is None else np.ascontiguousarray(mus, dtype=np.float64).reshape(len(fam), -1)
        if lam.shape[1] != self.problem.n_lambdas or nu.shape != lam.shape or (mu is not None and mu.shape != lam.shape):
            raise ValueError("lambdas, mus and nus must be [%d][%d]" % (len(fam), self.problem.n_lambdas))
        cp, keep = self._params(pr)
        out = np.empty(len(fam))
        self._check(self._lib.cafe_score_per_family_gain(self._h, C.byref(cp), len(fam), _p(fam, _i64p), _p(lam, _f64p),
                                                         None if mu is None else _p(mu, _f64p), _p(nu, _f64p), float(root_absent), _p(out, _f64p)))
        return out

    def gain_posterior(self, pr: Params, families, lambdas, mus, nus, root_absent: float = 0.0, want_posterior: bool = False) -> dict:
        """cafe_gain_posterior: under the gain model, entry i = families[i] under its own (lambdas, mus, nus)[i] (the arguments
        of score_per_family_gain), for every node: p_absent = P(size = 0 | counts), mean, p_gain = P(parent absent, node present
        | counts), p_loss = P(parent present, node absent | counts) -- NaN at the root -- all [n][n_nodes], and lnl [n], the
        sum-rule lnL whatever the context's root rule is.  want_posterior adds posterior [n][n_nodes][matrix_size]."""
        fam = np.ascontiguousarray(families, dtype=np.int64).reshape(-1)
        lam = np.ascontiguousarray(lambdas, dtype=np.float64).reshape(len(fam), -1)
        nu = np.ascontiguousarray(nus, dtype=np.float64).reshape(len(fam), -1)
        mu = None if mus is None else np.ascontiguousarray(mus, dtype=np.float64).reshape(len(fam), -1)
        if lam.shape[1] != self.problem.n_lambdas or nu.shape != lam.shape or (mu is not None and mu.shape != lam.shape):
            raise ValueError("lambdas, mus and nus must be [%d][%d]" % (len(fam), self.problem.n_lambdas))
        cp, keep = self._params(pr)
        n, nodes = len(fam), self.problem.n_nodes
        res = {"lnl": np.empty(n), "p_absent": np.empty((n, nodes)), "mean": np.empty((n, nodes)), "p_gain": np.empty((n, nodes)),
               "p_loss": np.empty((n, nodes))}
        if want_posterior:
            res["posterior"] = np.empty((n, nodes, self.problem.matrix_size))
        out = CafeGainPosteriorOut()
        for name, array in res.items():
            setattr(out, name, _p(array, _f64p))
        self._check(self._lib.cafe_gain_posterior(self._h, C.byref(cp), n, _p(fam, _i64p), _p(lam, _f64p), None if mu is None else _p(mu, _f64p),
                                                  _p(nu, _f64p), float(root_absent), C.byref(out)))
        return res

    def marginal_reconstruct(self, pr: Params, level: float = 0.95, alpha: float = 1.0) -> dict:
        """cafe_marginal_reconstruct: posterior size of every node under the scorer's model with pr's lambdas, categories,
        prior and error model.  Returns numpy arrays: mean, mode, lo, hi, p_increase, p_decrease [n_families][n_nodes],
        log_evidence and failed [n_families]; lo..hi is the equal-tailed interval at `level`."""
        cp, keep = self._params(pr, alpha)
        F, n = self.n_families, self.n_nodes
        res = {"mean": np.empty((F, n)), "mode": np.empty((F, n), dtype=np.int32), "lo": np.empty((F, n), dtype=np.int32),
               "hi": np.empty((F, n), dtype=np.int32), "p_increase": np.empty((F, n)), "p_decrease": np.empty((F, n)),
               "log_evidence": np.empty(F), "failed": np.empty(F, dtype=np.int32)}
        mo = CafeMarginalOut()
        for name, _ in CafeMarginalOut._fields_:
            setattr(mo, name, _p(res[name], _i32p if res[name].dtype == np.int32 else _f64p))
        self._check(self._lib.cafe_marginal_reconstruct(self._h, C.byref(cp), float(level), C.byref(mo)))
        return res

    def score_gradient(self, pr: Params, root_rule="max", alpha: float = 1.0, death_rates: Optional[bool] = None) -> dict:
        """cafe_score_gradient: every family's log likelihood and its derivative in the rates at pr.  root_rule "max"
        differentiates what score() returns per family, "sum" marginal_reconstruct's log_evidence.  Returns numpy arrays:
        family_lnl and failed [n_families], d_lambda [n_families][n_lambdas] (along lambda = mu unless death rates are set),
        d_mu of the same shape while death rates are set (death_rates: whether to ask for it; None asks the last
        set_death_rates of this object), d_multiplier [n_families][K] with the gamma model."""
        rule = {"max": CAFE_ROOT_MAX, "sum": CAFE_ROOT_SUM}.get(root_rule, root_rule)
        cp, keep = self._params(pr, alpha)
        F, nl = self.n_families, self.problem.n_lambdas
        res = {"family_lnl": np.empty(F), "d_lambda": np.empty((F, nl)), "failed": np.empty(F, dtype=np.int32)}
        if getattr(self, "_death_rates", False) if death_rates is None else death_rates:
            res["d_mu"] = np.empty((F, nl))
        if pr.multipliers is not None:
            res["d_multiplier"] = np.empty((F, len(pr.multipliers)))
        go = CafeGradientOut()
        for name, t in CafeGradientOut._fields_:
            if name in res:
                setattr(go, name, _p(res[name], t))
        self._check(self._lib.cafe_score_gradient(self._h, C.byref(cp), int(rule), C.byref(go)))
        return res

    def branch_scores_dim(self, pr: Params) -> int:
        """cafe_branch_scores_dim: the length P of the score vector for pr's model and this context's death rates."""
        cp, keep = self._params(pr)
        out = C.c_int32()
        self._check(self._lib.cafe_branch_scores_dim(self._h, C.byref(cp), C.byref(out)))
        return out.value

    def branch_scores(self, pr: Params, root_rule="max", alpha: float = 1.0, death_rates: Optional[bool] = None, per_family: bool = True,
                      gram: bool = True) -> dict:
        """cafe_branch_scores: score_gradient's derivative kept per branch, and the information of those scores.  Returns what
        score_gradient returns and, with per_family, rate [n_families][n_nodes] (d lnL_f / d log of a factor on both rates of
        the branch above the node; NaN at the root) and, while death rates are set, birth and death of the same shape (rate =
        birth + death); with gram, total [P], gram [P][P] and n_used over the score vector (branch scores, then d_lambda, d_mu,
        d_multiplier; P = branch_scores_dim)."""
        rule = {"max": CAFE_ROOT_MAX, "sum": CAFE_ROOT_SUM}.get(root_rule, root_rule)
        cp, keep = self._params(pr, alpha)
        F, nl, n = self.n_families, self.problem.n_lambdas, self.n_nodes
        two = getattr(self, "_death_rates", False) if death_rates is None else death_rates
        res = {"family_lnl": np.empty(F), "d_lambda": np.empty((F, nl)), "failed": np.empty(F, dtype=np.int32)}
        if two:
            res["d_mu"] = np.empty((F, nl))
        if pr.multipliers is not None:
            res["d_multiplier"] = np.empty((F, len(pr.multipliers)))
        if per_family:
            res["rate"] = np.empty((F, n))
            if two:
                res["birth"], res["death"] = np.empty((F, n)), np.empty((F, n))
        n_used = np.zeros(1, dtype=np.int64)
        if gram:
            P = self.branch_scores_dim(pr)
            res["total"], res["gram"] = np.empty(P), np.empty((P, P))
        bo = CafeBranchScoresOut()
        for name, t in CafeBranchScoresOut._fields_:
            if name in res:
                setattr(bo, name, _p(res[name], t))
        if gram:
            bo.n_used = _p(n_used, _i64p)
        self._check(self._lib.cafe_branch_scores(self._h, C.byref(cp), int(rule), C.byref(bo)))
        if gram:
            res["n_used"] = int(n_used[0])
        return res

    def gram_stats(self):
        """(HIP-event ms of the Gram launches of the last branch_scores -- 0 unless profiling was on --, the flops of their MFMAs)"""
        ms, fl = C.c_double(), C.c_double()
        self._check(self._lib.cafe_debug_gram(self._h, C.byref(ms), C.byref(fl)))
        return ms.value, fl.value

    def expected_events(self, pr: Params, alpha: float = 1.0) -> dict:
        """cafe_expected_events: the expected number of births (gains) and of deaths (losses) on the branch above every node
        given the leaf counts, under marginal_reconstruct's model.  Returns numpy arrays: gains and losses
        [n_families][n_nodes] (NaN at the root), log_evidence and failed [n_families]."""
        cp, keep = self._params(pr, alpha)
        F, n = self.n_families, self.n_nodes
        res = {"gains": np.empty((F, n)), "losses": np.empty((F, n)), "log_evidence": np.empty(F), "failed": np.empty(F, dtype=np.int32)}
        eo = CafeEventsOut()
        for name, t in CafeEventsOut._fields_:
            setattr(eo, name, _p(res[name], t))
        self._check(self._lib.cafe_expected_events(self._h, C.byref(cp), C.byref(eo)))
        return res

    def leaf_predictive(self, pr: Params, alpha: float = 1.0) -> dict:
        """cafe_leaf_predictive: the leave-one-out predictive distribution of every leaf count -- species l's count given the
        counts of every other species of the family, under marginal_reconstruct's model.  Returns numpy arrays: mean, sd,
        p_below, p_obs, p_above [n_families][n_taxa] (columns as the problem's counts; NaN where the distribution has no
        mass), log_evidence and failed [n_families].  p_below + p_obs and p_obs + p_above are the one-sided tail
        probabilities of the observed count."""
        cp, keep = self._params(pr, alpha)
        F, nt = self.n_families, self.problem.n_taxa
        res = {name: np.full((F, nt), np.nan) for name in ("mean", "sd", "p_below", "p_obs", "p_above")}
        res.update({"log_evidence": np.empty(F), "failed": np.empty(F, dtype=np.int32)})
        lo = CafeLeafPredictiveOut()
        for name, t in CafeLeafPredictiveOut._fields_:
            setattr(lo, name, _p(res[name], t))
        self._check(self._lib.cafe_leaf_predictive(self._h, C.byref(cp), C.byref(lo)))
        return res

    def branch_change(self, pr: Params, max_change: int = 10, level: float = 0.95, pmf: bool = True, alpha: float = 1.0) -> dict:
        """cafe_branch_change: the posterior of Delta = size(v) - size(parent(v)) on the branch above every node, under
        marginal_reconstruct's model.  Returns numpy arrays: pmf [n_families][n_nodes][2 max_change + 1] over
        -max_change..max_change (left out, and not allocated, with pmf=False), below and above (the mass beyond the band, each a
        sum of its own), mean (exact over the whole range), mode, lo, hi [n_families][n_nodes] (lo = -max_change - 1 /
        hi = max_change + 1: the interval's end lies in a tail), log_evidence and failed [n_families].  At the root and in a failed
        family the doubles are NaN and the integers CAFE_CHANGE_NONE."""
        cp, keep = self._params(pr, alpha)
        F, n, D = self.n_families, self.n_nodes, int(max_change)
        res = {"below": np.empty((F, n)), "above": np.empty((F, n)), "mean": np.empty((F, n)), "mode": np.empty((F, n), dtype=np.int32),
               "lo": np.empty((F, n), dtype=np.int32), "hi": np.empty((F, n), dtype=np.int32), "log_evidence": np.empty(F),
               "failed": np.empty(F, dtype=np.int32)}
        if pmf:
            res["pmf"] = np.empty((F, n, 2 * D + 1 if D >= 0 else 0))
        co = CafeBranchChangeOut()
        for name, t in CafeBranchChangeOut._fields_:
            if name in res:
                setattr(co, name, _p(res[name], t))
        self._check(self._lib.cafe_branch_change(self._h, C.byref(cp), D, float(level), C.byref(co)))
        return res

    def branch_change_band_ms(self):
        """summed HIP-event ms of the band kernel's launches of the last branch_change (0 unless profiling was on)"""
        ms = C.c_double()
        self._check(self._lib.cafe_debug_branch_change_band(self._h, C.byref(ms)))
        return ms.value

    def sample_histories(self, pr: Params, n_draws: int, seed: int, alpha: float = 1.0, sizes: bool = True) -> dict:
        """cafe_sample_histories: n_draws ancestral histories of every family from the posterior of marginal_reconstruct's
        model.  Returns numpy arrays: sizes int32 [n_draws][n_families][n_nodes] (left out with sizes=False: then only
        the counts leave the device), category int32 [n_draws][n_families], n_increase / n_decrease / net_change int64
        [n_draws][n_nodes], log_evidence and failed [n_families]."""
        cp, keep = self._params(pr, alpha)
        D, F, n = int(n_draws), self.n_families, self.n_nodes
        rows = D
        if not 1 <= D <= 65536:
            rows = 0                                             # the library rejects the call; nothing to allocate for it
        res = {"category": np.empty((rows, F), dtype=np.int32), "n_increase": np.empty((rows, n), dtype=np.int64),
               "n_decrease": np.empty((rows, n), dtype=np.int64), "net_change": np.empty((rows, n), dtype=np.int64),
               "log_evidence": np.empty(F), "failed": np.empty(F, dtype=np.int32)}
        if sizes:
            res["sizes"] = np.empty((rows, F, n), dtype=np.int32)
        ho = CafeHistoryOut()
        for name, t in CafeHistoryOut._fields_:
            if name in res:
                setattr(ho, name, _p(res[name], t))
        self._check(self._lib.cafe_sample_histories(self._h, C.byref(cp), D, int(seed), C.byref(ho)))
        return res

    def history_batches(self):
        """(column batches, draw passes per batch) of the last sample_histories under the workspace budget"""
        self._lib.cafe_debug_history_batches.restype = C.c_int
        self._lib.cafe_debug_history_batches.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        nb, npass = C.c_int32(), C.c_int32()
        self._check(self._lib.cafe_debug_history_batches(self._h, C.byref(nb), C.byref(npass)))
        return nb.value, npass.value

    def marginal_gemm_stats(self):
        """(summed HIP-event ms of the GEMM launches of the last marginal_reconstruct -- 0 unless profiling was on --, their flops)"""
        ms, fl = C.c_double(), C.c_double()
        self._check(self._lib.cafe_debug_marginal_gemm(self._h, C.byref(ms), C.byref(fl)))
        return ms.value, fl.value

    def root_max(self, lambdas) -> np.ndarray:
        """max_j L_root[j] per family under the plain lambdas (p-value path, probability.cpp:313, :399)."""
        lam = np.ascontiguousarray(lambdas, dtype=np.float64)
        cp = CafeParams()
        cp.model = CAFE_MODEL_BASE
        cp.lambdas = _p(lam, _f64p)
        cp.n_categories = 1
        out = np.empty(self.n_families)
        self._check(self._lib.cafe_root_max(self._h, C.byref(cp), _p(out, _f64p)))
        return out

    def pvalues(self, lambdas, n_simulations: int = 1000, seed: int = 1) -> np.ndarray:
        """compute_pvalues with the simulation on the device (probability.cpp:418): against the reference's own sample the
        agreement is statistical, not draw-for-draw; the device's sample itself is a function of the seed that
        tests/test_pvalues_replay.py replays draw for draw (tests/pvalues_ref.py) and checks stage by stage."""
        lam = np.ascontiguousarray(lambdas, dtype=np.float64)
        cp = CafeParams()
        cp.model = CAFE_MODEL_BASE
        cp.lambdas = _p(lam, _f64p)
        cp.n_categories = 1
        out = np.empty(self.n_families)
        self._check(self._lib.cafe_pvalues(self._h, C.byref(cp), n_simulations, seed, _p(out, _f64p)))
        return out

    def pvalues_stages(self, lambdas, n_simulations: int = 1000, seed: int = 1) -> dict:
        """One pvalues() call that also reads back what its stages left on the device (cafe_debug_pvalues_stages), Fs = R *
        n_simulations: sizes int32 [n_nodes][Fs], counts int32 [n_taxa][Fs] (the simulated families' leaf counts as their
        context reads them), cond_unsorted / cond_sorted [R][n_simulations] (their root maxima either side of the sort),
        observed [n_families] (the root maxima of the listed families), pvalues [n_families]."""
        f = self._lib.cafe_debug_pvalues_stages
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(CafeParams), C.c_int32, C.c_uint64, C.POINTER(CafePvalueStages), _f64p]
        lam = np.ascontiguousarray(lambdas, dtype=np.float64)
        cp = CafeParams()
        cp.model = CAFE_MODEL_BASE
        cp.lambdas = _p(lam, _f64p)
        cp.n_categories = 1
        pb = self.problem
        Fs = max(0, self.R * n_simulations)                  # (an invalid n_simulations is refused before anything is written)
        res = {"sizes": np.full((self.n_nodes, Fs), -1, dtype=np.int32), "counts": np.full((pb.n_taxa, Fs), -1, dtype=np.int32),
               "cond_unsorted": np.full((self.R, max(0, n_simulations)), np.nan), "cond_sorted": np.full((self.R, max(0, n_simulations)), np.nan),
               "observed": np.full(self.n_families, np.nan), "pvalues": np.full(self.n_families, np.nan)}
        st = CafePvalueStages(_p(res["sizes"], _i32p), _p(res["counts"], _i32p), _p(res["cond_unsorted"], _f64p),
                              _p(res["cond_sorted"], _f64p), _p(res["observed"], _f64p))
        self._check(f(self._h, C.byref(cp), n_simulations, seed, C.byref(st), _p(res["pvalues"], _f64p)))
        return res

    def reconstruct(self, lambdas, root_prior, multipliers=None) -> np.ndarray:
        """Pupko joint reconstruction -> int32 [K][n_families][n_nodes] (gene_family_reconstructor.cpp:13-165).
        root_prior[j] = compute(j), j = 0..min(M, R)."""
        lam = np.ascontiguousarray(lambdas, dtype=np.float64)
        rp = np.ascontiguousarray(root_prior, dtype=np.float32)
        if len(rp) < min(self.M, self.R) + 1:
            raise CafeError("root_prior needs min(M, R) + 1 entries")
        cp = CafeParams()
        cp.lambdas = _p(lam, _f64p)
        K = 1
        mult = None
        if multipliers is not None:
            mult = np.ascontiguousarray(multipliers, dtype=np.float64)
            K = len(mult)
            cp.model = CAFE_MODEL_GAMMA
            cp.multipliers = _p(mult, _f64p)
        else:
            cp.model = CAFE_MODEL_BASE
        cp.n_categories = K
        out = np.empty((K, self.n_families, self.n_nodes), dtype=np.int32)
        self._check(self._lib.cafe_reconstruct(self._h, C.byref(cp), _p(rp, _f32p), _p(out, _i32p)))
        return out

    def branch_probabilities(self, lambdas, sizes) -> np.ndarray:
        """compute_viterbi_sum for every (family, node); NaN = invalid (gene_family_reconstructor.cpp:361-400)."""
        lam = np.ascontiguousarray(lambdas, dtype=np.float64)
        sz = np.ascontiguousarray(sizes, dtype=np.int32)
        assert sz.shape == (self.n_families, self.n_nodes)
        cp = CafeParams()
        cp.model = CAFE_MODEL_BASE
        cp.lambdas = _p(lam, _f64p)
        cp.n_categories = 1
        out = np.empty((self.n_families, self.n_nodes))
        self._check(self._lib.cafe_branch_probabilities(self._h, C.byref(cp), _p(sz, _i32p), _p(out, _f64p)))
        return out

    def score_partial(self, pr: Params, device_ptr: int, stream: int = 0, alpha: float = 1.0):
        """Enqueue the shard's work; {sum lnL, rejects} lands in 2 doubles of device memory."""
        cp, keep = self._params(pr, alpha)
        self._check(self._lib.cafe_score_partial(self._h, C.byref(cp), C.c_void_p(device_ptr), C.c_void_p(stream)))

    def finish(self, host_pair) -> float:
        a = np.ascontiguousarray(host_pair, dtype=np.float64)
        return self._lib.cafe_finish_partial(_p(a, _f64p))

    def matrix(self, node: int, category: int = 0) -> np.ndarray:
        n = self._lib.cafe_matrix_size(self._h)
        out = np.empty((n, n))
        self._check(self._lib.cafe_get_matrix(self._h, node, category, _p(out, _f64p), out.size))
        return out

    def root_likelihoods(self, family: int, category: int = 0) -> np.ndarray:
        out = np.empty(self.R)
        self._check(self._lib.cafe_get_root_likelihoods(self._h, family, category, _p(out, _f64p), out.size))
        return out

    def stats(self) -> dict:
        st = CafeStats()
        self._check(self._lib.cafe_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def extents(self, node: int, category: int = 0):
        """(matrix extents [blocks or N][2], panel tile extents [tiles][2] or None) of the last call (cafe_get_extents)."""
        n = self._lib.cafe_matrix_size(self._h)
        m = np.zeros((max(n, (n + 14) // 16), 2), dtype=np.int32)
        pt = np.zeros((self.n_families // 128 + 2, 2), dtype=np.int32)
        nt = C.c_int32()
        self._check(self._lib.cafe_get_extents(self._h, node, category, _p(m, _i32p), m.size, _p(pt, _i32p), pt.size, C.byref(nt)))
        leaf = self.problem.leaf_taxon[node] >= 0
        return (m[:n] if leaf else m[:(n - 1 + 15) // 16]), (pt[:nt.value] if nt.value else None)

    def column_extents(self, node: int, category: int = 0) -> np.ndarray:
        """Per-column zero extents [columns][2] of an interior non-root node's panel in the last call (diagnostic)."""
        self._lib.cafe_debug_column_extents.restype = C.c_int
        self._lib.cafe_debug_column_extents.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _i32p, C.c_size_t, C.POINTER(C.c_int64)]
        out = np.zeros((self.n_families + 256, 2), dtype=np.int32)
        n = C.c_int64()
        self._check(self._lib.cafe_debug_column_extents(self._h, node, category, _p(out, _i32p), out.size, C.byref(n)))
        return out[:n.value]

    def panel_bounds(self, node: int, category: int = 0) -> np.ndarray:
        """Magnitude bounds [tiles][row steps] of an interior non-root node's panel in the last call: an upper bound of log2 of
        every computed entry of rows 4 r .. 4 r + 3 of a 128-column tile, -inf where all are zero (cafe_debug_panel_bounds)."""
        f = self._lib.cafe_debug_panel_bounds
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _f64p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        nt, nr = C.c_int32(), C.c_int32()
        self._check(f(self._h, node, category, None, 0, C.byref(nt), C.byref(nr)))
        out = np.zeros((nt.value, nr.value), dtype=np.float64)
        self._check(f(self._h, node, category, _p(out, _f64p), out.size, C.byref(nt), C.byref(nr)))
        return out

    def set_level_tiles(self, tiles: int) -> None:
        """Column tiles per workgroup of the per-level interval / bound kernel in the following calls: 1, 2 or 4, 0 = chosen per
        level (cafe_debug_level_tiles).  Diagnostic: nothing the library returns depends on it."""
        self._lib.cafe_debug_level_tiles.restype = C.c_int
        self._lib.cafe_debug_level_tiles.argtypes = [C.c_void_p, C.c_int]
        self._check(self._lib.cafe_debug_level_tiles(self._h, tiles))

    def magnitude_tables(self, which: str, node: int, category: int = 0) -> np.ndarray:
        """One magnitude table of the matrix of the branch above `node` in the last call, as the device wrote it (int32, units
        of 1/256 of log2, MAG_NONE where everything the entry stands for is zero): "a16" [k-steps][16-row blocks] and "t4"
        [k-steps][row steps] of an interior branch, "lt" [counts 0 .. M][row steps] of a leaf branch
        (cafe_debug_magnitude_tables)."""
        f = self._lib.cafe_debug_magnitude_tables
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _i32p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32]
        w = {"a16": 0, "t4": 1, "lt": 2}[which]
        n0, n1 = C.c_int32(), C.c_int32()
        self._check(f(self._h, w, -1, None, 0, C.byref(n0), C.byref(n1), node, category))
        out = np.zeros((n0.value, n1.value), dtype=np.int32)
        self._check(f(self._h, w, -1, _p(out, _i32p), out.size, C.byref(n0), C.byref(n1), node, category))
        return out

    def k_ranges(self, node: int, category: int = 0) -> np.ndarray:
        """K ranges [tiles][16-row blocks][2] (first / last k-step, 4 deep; first > last: none) of the K2 op of the branch above
        an interior non-root node in the last call (cafe_debug_k_ranges)."""
        f = self._lib.cafe_debug_k_ranges
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _i32p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        nt, nb = C.c_int32(), C.c_int32()
        self._check(f(self._h, node, category, None, 0, C.byref(nt), C.byref(nb)))
        out = np.zeros((nt.value, nb.value, 2), dtype=np.int32)
        self._check(f(self._h, node, category, _p(out, _i32p), out.size, C.byref(nt), C.byref(nb)))
        return out

    def narrowed_extents(self, node: int, category: int = 0) -> np.ndarray:
        """Narrowed hulls [tiles][2] of an interior non-root node's panel in the last call: the structural hull of each
        128-column tile cut back over the rows the magnitude bounds prove to be computed zeros (first > last: the whole tile);
        the structural hulls themselves under CAFE_NO_NARROW=1 or without bounds (cafe_debug_narrowed_extents)."""
        f = self._lib.cafe_debug_narrowed_extents
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _i32p, C.c_size_t, C.POINTER(C.c_int32)]
        out = np.zeros(((self.n_families + 256) // 128 + 2, 2), dtype=np.int32)
        nt = C.c_int32()
        self._check(f(self._h, node, category, _p(out, _i32p), out.size, C.byref(nt)))
        return out[:nt.value]

    def leaf_transposes(self):
        """(leaf branches with a transposed copy of their matrix for the assemble passes, whether the last call used them)."""
        self._lib.cafe_debug_leaf_transposes.restype = C.c_int
        self._lib.cafe_debug_leaf_transposes.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        n, used = C.c_int32(), C.c_int32()
        self._check(self._lib.cafe_debug_leaf_transposes(self._h, C.byref(n), C.byref(used)))
        return n.value, bool(used.value)

    def launch_flops(self):
        """Per K2 launch of the last call: (executed flops, flops over all K tiles, tile height in 16-row blocks)."""
        n = int(self.stats()["gemm_launches"])
        ex, al, mi = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
        self._check(self._lib.cafe_debug_launch_flops(self._h, _p(ex, _f64p), _p(al, _f64p), _p(mi, _i32p), n))
        return ex, al, mi

    def plan_check(self):
        """(launches of the last call that ran from planned tile lists, worst modelled workgroup load / mean); raises when a
        list does not cover its launch's tiles exactly once with the K ranges the extents give."""
        n, w = C.c_int32(), C.c_double()
        self._lib.cafe_debug_plan_check.restype = C.c_int
        self._lib.cafe_debug_plan_check.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        self._check(self._lib.cafe_debug_plan_check(self._h, C.byref(n), C.byref(w)))
        return n.value, w.value

    def executed_flops(self) -> float:
        """Flops the K2 launches of the last call really ran (K tiles outside matrix extent x panel extent are skipped)."""
        v = C.c_double()
        self._check(self._lib.cafe_executed_flops(self._h, C.byref(v)))
        return v.value

    def issued_flops(self) -> float:
        """Flops of the MFMAs the K2 launches of the last call issued: executed_flops() less the k-steps whose products
        underflow below the smallest denormal (cafe_issued_flops)."""
        self._lib.cafe_issued_flops.restype = C.c_int
        self._lib.cafe_issued_flops.argtypes = [C.c_void_p, _f64p]
        v = C.c_double()
        self._check(self._lib.cafe_issued_flops(self._h, C.byref(v)))
        return v.value

    def tile_range_flops(self) -> float:
        """The same with every row block of a tile counted over the tile's whole K range (cafe_debug_tile_range_flops)."""
        self._lib.cafe_debug_tile_range_flops.restype = C.c_int
        self._lib.cafe_debug_tile_range_flops.argtypes = [C.c_void_p, _f64p]
        v = C.c_double()
        self._check(self._lib.cafe_debug_tile_range_flops(self._h, C.byref(v)))
        return v.value

    def debug_stamps(self, words: int) -> np.ndarray:
        out = np.zeros(words, dtype=np.uint64)
        self._check(self._lib.cafe_debug_stamps(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), words))
        return out

    def force_tile(self, mi: int):
        """Diagnostic: K2 row tile of 16*mi rows for every launch (0: chosen per launch)."""
        self._check(self._lib.cafe_debug_force_tile(self._h, mi))

    def set_profiling(self, on: bool):
        self._check(self._lib.cafe_set_profiling(self._h, 1 if on else 0))

    def debug_fail_next(self, n: int = 1):
        """Test hook: the n-th next call of this context fails with CAFE_ERR_DEVICE in the middle of its enqueue."""
        self._check(self._lib.cafe_debug_fail_next(self._h, n))

    def set_death_rates(self, mus):
        """cafe_set_death_rates: from now on every call of this context scores the birth-death process with birth rate
        lambdas[i] and death rate mus[i] (one per lambda index); None restores lambda = mu."""
        if mus is None:
            self._check(self._lib.cafe_set_death_rates(self._h, None))
            self._death_rates = False
            return
        mu = np.ascontiguousarray(np.atleast_1d(mus), dtype=np.float64)
        pb = getattr(self, "problem", None)                  # (a shard borrowed from a Sharded object does not know its problem)
        if pb is not None and mu.shape != (pb.n_lambdas,):
            raise ValueError("mus must have %d entries" % pb.n_lambdas)
        self._check(self._lib.cafe_set_death_rates(self._h, _p(mu, _f64p)))
        self._death_rates = True

    def set_root_rule(self, rule):
        """cafe_set_root_rule: "max" (the default, the reference's max_s(L_s prior_s)) or "sum" (the marginal likelihood
        sum_s L_s prior_s) -- what score(), score_partial(), family_results() and score_per_family[_lm]() make of a family's
        root vector from now on."""
        self._check(self._lib.cafe_set_root_rule(self._h, int({"max": CAFE_ROOT_MAX, "sum": CAFE_ROOT_SUM}.get(rule, rule))))

    def root_rule(self) -> str:
        return "sum" if self._lib.cafe_get_root_rule(self._h) == CAFE_ROOT_SUM else "max"

    def root_posterior(self, pr: Params, alpha: float = 1.0) -> dict:
        """cafe_root_posterior: the posterior of every family's root size under the sum rule, on the scorer's own prune.
        Returns total [R] (the sum over the families that did not fail of P(root size = j + 1 | data)), n_used (int), mean,
        mode, log_evidence and failed [n_families] and, with the gamma model, category_posterior [n_families][K].
        total / n_used is the EM update of the root distribution."""
        cp, keep = self._params(pr, alpha)
        F = self.n_families
        res = {"total": np.empty(self.R), "mean": np.empty(F), "mode": np.empty(F, dtype=np.int32), "log_evidence": np.empty(F),
               "failed": np.empty(F, dtype=np.int32)}
        if pr.multipliers is not None:
            res["category_posterior"] = np.empty((F, len(pr.multipliers)))
        n_used = np.zeros(1, dtype=np.int64)
        ro = CafeRootPosteriorOut()
        for name, t in CafeRootPosteriorOut._fields_:
            if name in res:
                setattr(ro, name, _p(res[name], t))
        ro.n_used = _p(n_used, _i64p)
        self._check(self._lib.cafe_root_posterior(self._h, C.byref(cp), C.byref(ro)))
        res["n_used"] = int(n_used[0])
        return res

    def set_graphs(self, on: bool):
        """False: enqueue every call launch by launch instead of replaying its captured hipGraph."""
        self._check(self._lib.cafe_set_graphs(self._h, 1 if on else 0))


class _Borrowed(Context):
    """A shard's cafe_ctx owned by a Sharded object: statistics and introspection only."""

    def __init__(self, lib, handle, n_families):
        self._lib, self._h, self.n_families = lib, handle, n_families

    def close(self):
        self._h = None


class Sharded:
    """cafe_create_sharded: one process, several GPUs -- family shards, one host thread and stream per device, one
    RCCL all-reduce per scorer call."""

    def __init__(self, pb: Problem, devices, max_categories: int = 1, dedup: bool = True, subtree_dedup: bool = True):
        self._lib = load()
        keep = []
        cp = _c_problem(pb, keep, max_categories, 0, (0 if dedup else CAFE_FLAG_NO_DEDUP) | (0 if subtree_dedup else CAFE_FLAG_NO_SUBTREE_DEDUP))
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        err = C.create_string_buffer(512)
        self._h = self._lib.cafe_create_sharded(C.byref(cp), _p(dev, _i32p), len(dev), err, 512)
        if not self._h:
            raise CafeError(err.value.decode() or "cafe_create_sharded failed")
        self.n_families = pb.n_families
        self.size = self._lib.cafe_sharded_size(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cafe_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise CafeError("code %d: %s" % (rc, self._lib.cafe_sharded_last_error(self._h).decode()))

    def score(self, pr: Params, alpha: float = 1.0, per_family: bool = False):
        cp, keep = _c_params(pr, alpha)
        out = C.c_double()
        self._check(self._lib.cafe_sharded_score(self._h, C.byref(cp), C.byref(out), None))
        if not per_family:
            return out.value
        return out.value, self.family_results(len(pr.multipliers) if pr.multipliers is not None else 0)

    def family_results(self, K: int = 0):
        F = self.n_families
        fo = CafeFamilyOut()
        res = {"family_lnl": np.empty(F), "failed": np.empty(F, dtype=np.int32)}
        fo.family_lnl = _p(res["family_lnl"], _f64p)
        fo.failed = _p(res["failed"], _i32p)
        if K > 0:
            res["category_likelihood"] = np.empty((F, K))
            res["family_likelihood"] = np.empty(F)
            fo.category_likelihood = _p(res["category_likelihood"], _f64p)
            fo.family_likelihood = _p(res["family_likelihood"], _f64p)
        self._check(self._lib.cafe_sharded_family_results(self._h, C.byref(fo)))
        return res

    def set_root_rule(self, rule):
        """Context.set_root_rule on every shard (the C ABI has no sharded entry: the rule is a property of each shard's context)."""
        for r in range(self.size):
            self.shard(r).set_root_rule(rule)

    def shard(self, r: int) -> Context:
        h = self._lib.cafe_sharded_context(self._h, r)
        if not h:
            raise CafeError("no shard %d" % r)
        return _Borrowed(self._lib, h, 0)


def build_matrices(n: int, lambdas, ts, device: int = 0, layout: int = 0) -> np.ndarray:
    lam = np.ascontiguousarray(lambdas, dtype=np.float64)
    t = np.ascontiguousarray(ts, dtype=np.float64)
    out = np.empty((len(lam), n, n))
    rc = load().cafe_build_matrices(device, n, len(lam), _p(lam, _f64p), _p(t, _f64p), layout, _p(out, _f64p))
    if rc:
        raise CafeError("cafe_build_matrices failed with code %d" % rc)
    return out


def debug_sort_rows(values, device: int = 0) -> np.ndarray:
    """cafe_debug_sort_rows: every row of values [rows][n] sorted ascending by cafe_pvalues' sort kernel, launched as it
    launches it; returns a new array."""
    L = load()
    L.cafe_debug_sort_rows.restype = C.c_int
    L.cafe_debug_sort_rows.argtypes = [C.c_int32, _f64p, C.c_int32, C.c_int32]
    out = np.array(values, dtype=np.float64, order="C")
    if out.ndim != 2:
        raise ValueError("values must be [rows][n]")
    rc = L.cafe_debug_sort_rows(device, _p(out, _f64p), out.shape[0], out.shape[1])
    if rc:
        raise CafeError("cafe_debug_sort_rows failed with code %d" % rc)
    return out


def debug_tree_pvalue(observed, cond, device: int = 0) -> np.ndarray:
    """cafe_debug_tree_pvalue: cafe_pvalues' p-value kernel on observed [F] and cond [R][n] (rows sorted ascending)."""
    L = load()
    L.cafe_debug_tree_pvalue.restype = C.c_int
    L.cafe_debug_tree_pvalue.argtypes = [C.c_int32, _f64p, C.c_int64, _f64p, C.c_int32, C.c_int32, _f64p]
    obs = np.ascontiguousarray(observed, dtype=np.float64)
    c = np.ascontiguousarray(cond, dtype=np.float64)
    if obs.ndim != 1 or c.ndim != 2:
        raise ValueError("observed must be [F] and cond [R][n]")
    out = np.full(len(obs), np.nan)
    rc = L.cafe_debug_tree_pvalue(device, _p(obs, _f64p), len(obs), _p(c, _f64p), c.shape[0], c.shape[1], _p(out, _f64p))
    if rc:
        raise CafeError("cafe_debug_tree_pvalue failed with code %d" % rc)
    return out


def bd_rates(lam: float, mu: float, t: float):
    """cafe_bd_rates: (alpha, beta, zero) of the quantized key (lambda, mu, t).  Host code: needs no GPU."""
    out = np.empty(3)
    rc = load().cafe_bd_rates(float(lam), float(mu), float(t), _p(out, _f64p))
    if rc:
        raise CafeError("cafe_bd_rates failed with code %d" % rc)
    return float(out[0]), float(out[1]), bool(out[2])


def bd_gain_row0(lam: float, mu: float, nu: float, t: float, n: int):
    """cafe_bd_gain_row0: (row 0 of the gain model's matrix for the quantized key, columns 0..n-1; r = nu / lambda).  Host
    code: needs no GPU."""
    out, r = np.empty(int(n)), np.empty(1)
    rc = load().cafe_bd_gain_row0(float(lam), float(mu), float(nu), float(t), int(n), _p(out, _f64p), _p(r, _f64p))
    if rc != 0:
        raise CafeError("cafe_bd_gain_row0 failed with code %d" % rc)
    return out, float(r[0])


def bd_rates_grad(lam: float, mu: float, t: float):
    """cafe_bd_rates_grad: (d alpha / d lambda, d alpha / d mu, d beta / d lambda, d beta / d mu) at the quantized key
    (lambda, mu, t).  Host code: needs no GPU."""
    out = np.empty(4)
    rc = load().cafe_bd_rates_grad(float(lam), float(mu), float(t), _p(out, _f64p))
    if rc:
        raise CafeError("cafe_bd_rates_grad failed with code %d" % rc)
    return tuple(float(x) for x in out)


def weighted_gram(S, w, device: int = 0):
    """cafe_weighted_gram: (S diag(w) S^T [p][p], S w [p]) of S [p][n] on the device's fp64 MFMA."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    p, n = S.shape
    if w.shape != (n,):
        raise ValueError("w must have one entry per column of S")
    gram, total = np.empty((p, p)), np.empty(p)
    rc = load().cafe_weighted_gram(int(device), p, n, _p(S, _f64p), _p(w, _f64p), _p(gram, _f64p), _p(total, _f64p))
    if rc != 0:
        raise CafeError("cafe_weighted_gram failed with code %d" % rc)
    return gram, total


def bd_rates_events(lam: float, mu: float, t: float):
    """cafe_bd_rates_events: (da, db, dc) of the births tag, then (da, db, dc) of the deaths tag, at the quantized key
    (lambda, mu, t).  Host code: needs no GPU."""
    out = np.empty(6)
    rc = load().cafe_bd_rates_events(float(lam), float(mu), float(t), _p(out, _f64p))
    if rc:
        raise CafeError("cafe_bd_rates_events failed with code %d" % rc)
    return tuple(float(x) for x in out)


def build_matrices_lm(n: int, lambdas, mus, ts, device: int = 0, layout: int = 0) -> np.ndarray:
    """cafe_build_matrices_lm: the two-rate kernel's matrices for (lambdas[i], mus[i], ts[i]), always P[s][c] row-major."""
    lam = np.ascontiguousarray(lambdas, dtype=np.float64)
    mu = np.ascontiguousarray(mus, dtype=np.float64)
    t = np.ascontiguousarray(ts, dtype=np.float64)
    if not (lam.shape == mu.shape == t.shape):
        raise ValueError("lambdas, mus and ts must have the same length")
    out = np.empty((len(lam), n, n))
    rc = load().cafe_build_matrices_lm(device, n, len(lam), _p(lam, _f64p), _p(mu, _f64p), _p(t, _f64p), layout, _p(out, _f64p))
    if rc:
        raise CafeError("cafe_build_matrices_lm failed with code %d" % rc)
    return out


def _simulate(call, pb: Problem, lambdas, max_family_size: int, root_size, seed: int, chunk_size: int = 50, chunk_multiplier=None,
              error_model=None, error_model_max_size: int = 0, device: int = 0, workspace_limit: int = 0, node_sizes: bool = True):
    """What simulate and simulate_lm share: the cafe_sim_problem block and the outputs.  call(problem, seed, leaf, nodes, err,
    errlen) is the C entry, with whatever else it takes already bound."""
    keep = []

    def k(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a
    lam = k(np.atleast_1d(lambdas), np.float64)
    roots = k(root_size, np.int32).reshape(-1)
    F = len(roots)
    cp = CafeSimProblem()
    cp.n_nodes = pb.n_nodes
    cp.parent = _p(k(pb.parent, np.int32), _i32p)
    cp.branch_length = _p(k(pb.branch_length, np.float64), _f64p)
    cp.lambda_index = _p(k(pb.lambda_index, np.int32), _i32p)
    cp.leaf_taxon = _p(k(pb.leaf_taxon, np.int32), _i32p)
    cp.n_taxa = pb.n_taxa
    cp.n_lambdas = len(lam)
    cp.lambdas = _p(lam, _f64p)
    cp.max_family_size = max_family_size
    cp.n_families = F
    cp.root_size = _p(roots, _i32p)
    cp.chunk_size = chunk_size
    if chunk_multiplier is not None:
        cm = k(chunk_multiplier, np.float64).reshape(-1)
        n_chunks = (F + chunk_size - 1) // chunk_size if chunk_size > 0 else min(F, 1)
        if len(cm) < n_chunks:
            raise CafeError("chunk_multiplier needs %d entries" % n_chunks)
        cp.chunk_multiplier = _p(cm, _f64p)
    if error_model is not None:
        em = k(error_model, np.float64)
        if em.ndim != 2 or em.shape[0] < max_family_size:
            raise CafeError("error_model needs [S][n_deviations] entries")
        em = k(em[:max_family_size], np.float64)
        cp.n_deviations = em.shape[1]
        cp.error_model = _p(em, _f64p)
        cp.error_model_max_size = error_model_max_size
    cp.device = device
    cp.workspace_limit = workspace_limit
    leaf = np.empty((F, pb.n_taxa), dtype=np.int32)
    nodes = np.empty((F, pb.n_nodes), dtype=np.int32) if node_sizes else None
    err = C.create_string_buffer(512)
    rc = call(C.byref(cp), seed, _p(leaf, _i32p), _p(nodes, _i32p), err, 512)
    if rc:
        raise CafeError("code %d: %s" % (rc, err.value.decode()))
    return leaf, nodes


def simulate(pb: Problem, lambdas, max_family_size: int, root_size, seed: int, chunk_size: int = 50, chunk_multiplier=None,
             error_model=None, error_model_max_size: int = 0, device: int = 0, workspace_limit: int = 0, node_sizes: bool = True):
    """cafe_simulate: gene families simulated down pb's tree (its parent / branch_length / lambda_index / leaf_taxon; its
    families are not read) from root_size[F], every child size drawn from the order-S transition matrices of the chunk's
    lambdas * chunk_multiplier[f // chunk_size].  error_model: [S][n_deviations] table of get_probs(c), with
    error_model_max_size = error_model::get_max_family_size().  Returns (leaf_counts int32 [F][n_taxa], node_sizes int32
    [F][n_nodes] or None)."""
    return _simulate(load().cafe_simulate, pb, lambdas, max_family_size, root_size, seed, chunk_size, chunk_multiplier, error_model,
                     error_model_max_size, device, workspace_limit, node_sizes)


def simulate_lm(pb: Problem, lambdas, mus, max_family_size: int, root_size, seed: int, **kwargs):
    """cafe_simulate_lm: simulate() under separate birth and death rates, mus[n_lambdas] beside lambdas (a chunk multiplier
    scales both).  mus=None passes NULL, which is cafe_simulate.  Keyword arguments and the result are simulate()'s."""
    mu = None
    if mus is not None:
        mu = np.ascontiguousarray(np.atleast_1d(mus), dtype=np.float64)
        if mu.shape != np.atleast_1d(lambdas).shape:
            raise CafeError("mus needs one entry per lambda")
    return _simulate(lambda cp, *rest: load().cafe_simulate_lm(cp, _p(mu, _f64p), *rest), pb, lambdas, max_family_size, root_size, seed, **kwargs)


def probe_fp64_mfma(device: int = 0) -> float:
    v = C.c_double()
    rc = load().cafe_probe_fp64_mfma(device, C.byref(v))
    if rc:
        raise CafeError("cafe_probe_fp64_mfma failed with code %d" % rc)
    return v.value
