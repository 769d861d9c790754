"""cafe_expected_events (csrc/events.hip) at the smallest shapes at which each of its kernels can go wrong: the inputs of
tests/test_gradient_shapes.py, whose kernels it shares or mirrors.

Tree: a cherry, a polytomy of 7 leaves, a clade with an interior child and a leaf under the root; two lambda classes.  (M, R) in
PAIRS: M in {15, 16, 63, 64, 65} -- either side of the scan's 8-row blocks, the leaf filter's 32-column tiles and 64-row blocks,
the GEMM's 16-deep K step and 64-row tile -- with R below and above M.  Families: counts 0 and M at leaves under a 3-tap error
model (taps fall outside [0, M]), every leaf at M, duplicates.  Models (CONFIGS of that file): base with lambda = mu; gamma K = 3
with the error model and death rates four times the lambdas; base with the error model and death rates a quarter of them.
Column counts 1, 127, 128, 129 and 300 distinct families; a workspace_limit that forces three column batches.

Reference and bound are test_events_gpu's: events_ref.reference, |got - ref| <= 1e-12 + 1e-10 c |ref| with c = 1 (sums of
non-negative terms; the CPU test asserts that the reference reports no cancellation on these inputs).

The CPU tests say what the GPU tests can see: the four deliberately wrong statements of the reference (gains and losses
swapped, the dc term dropped, c tied to (1 - a)(1 - b), the b term shifted by one instead of two) are each told from the right
one, by more than 100 x the bound, on every input set."""
import functools

import numpy as np
import pytest

import events_ref as ER
from test_gradient_shapes import COLUMNS, CONFIGS, PAIRS, _K, _params, _problem, kBN

C_BOUND = 1.0


@functools.lru_cache(maxsize=None)
def _pair_case(M, R, config):
    cfg = CONFIGS[config]
    pb = _problem(M, R, err=cfg["err"])
    pr = _params(pb, cfg)
    return pb, pr, cfg["mus"], ER.reference(pb, pr, cfg["mus"], route="filters")


@functools.lru_cache(maxsize=None)
def _column_case(n):
    cfg = CONFIGS["gamma_err_rho_0.25"]
    pb = _problem(40, 30, n=n, seed=n, err=True, distinct=True)
    pr = _params(pb, cfg)
    return pb, pr, cfg["mus"], ER.reference(pb, pr, cfg["mus"], route="filters")


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_reference_reports_no_cancellation(config):
    worst = max(ER.worst_cancellation(_pair_case(M, R, config)[3]) for M, R in PAIRS)
    assert worst <= C_BOUND + 1e-12
    for M, R in PAIRS[::3]:                                  # the other statement, on a third of the pairs
        pb, pr, mus, ref = _pair_case(M, R, config)
        ER.close(ER.reference(pb, pr, mus, route="rows"), ref, C_BOUND, "rows against filters M %d R %d %s" % (M, R, config))


@pytest.mark.parametrize("M,R", PAIRS)
def test_the_inputs_tell_a_wrong_statement_from_the_right_one(M, R):
    for config in sorted(CONFIGS):
        pb, pr, mus, ref = _pair_case(M, R, config)
        assert not ref["failed"].any()
        for name in ER.MUTANTS:
            mut = ER.reference(pb, pr, mus, mutant=name)
            ratio = max(np.nanmax(np.abs(mut[k] - ref[k]) / (1e-12 + 1e-10 * C_BOUND * np.abs(ref[k]))) for k in ER.KEYS)
            assert ratio > 100, (name, M, R, config, ratio)
            with pytest.raises(AssertionError):
                ER.close(mut, ref, C_BOUND, name)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _run(capi, pb, pr, mus, ref, label, **ctx_args):
    ctx = capi.Context(pb, max_categories=_K(pr), **ctx_args)
    try:
        ctx.set_death_rates(mus)
        got = ctx.expected_events(pr, alpha=0.7)
    finally:
        ctx.close()
    ER.close(got, ref, C_BOUND, label)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("M,R", PAIRS)
def test_every_pair_and_model(capi, M, R, config):
    pb, pr, mus, ref = _pair_case(M, R, config)
    got = _run(capi, pb, pr, mus, ref, "M %d R %d %s" % (M, R, config))
    assert not got["failed"].any()
    for key in ER.KEYS:                                      # duplicate families get equal rows
        assert np.array_equal(got[key][4], got[key][2], equal_nan=True) and np.array_equal(got[key][5], got[key][0], equal_nan=True), key


@pytest.mark.gpu
@pytest.mark.parametrize("n", COLUMNS)
def test_column_counts_around_the_tile(capi, n):
    pb, pr, mus, ref = _column_case(n)
    assert len(np.unique(pb.counts, axis=0)) == n
    _run(capi, pb, pr, mus, ref, "%d distinct families" % n)


def _per_col(pb, K):
    """expected_events_impl's own workspace formula: bytes per column"""
    nI = int((pb.leaf_taxon < 0).sum())
    rows = pb.matrix_size
    return (3 * nI * rows + 5 * rows + K + 2 * pb.n_nodes + 2) * 8


@pytest.mark.gpu
def test_three_column_batches_change_no_bit(capi):
    pb, pr, mus, ref = _column_case(300)
    per_col = _per_col(pb, 3)
    limit = kBN * per_col + per_col // 2
    assert limit // per_col // kBN * kBN == kBN and -(-300 // kBN) == 3
    want = _run(capi, pb, pr, mus, ref, "one batch")
    got = _run(capi, pb, pr, mus, ref, "three batches", workspace_limit=limit)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key


@pytest.mark.gpu
def test_the_gemm_count_is_the_two_rate_gradients(capi):
    """up 1 + down 1 + 2 per interior branch: cafe_debug_marginal_gemm reports the flops cafe_score_gradient reports with death
    rates set"""
    pb, pr, mus, _ = _column_case(128)
    ctx = capi.Context(pb, max_categories=_K(pr))
    try:
        ctx.set_death_rates(mus)
        ctx.expected_events(pr, alpha=0.7)
        ev = ctx.marginal_gemm_stats()
        ctx.score_gradient(pr, "sum", alpha=0.7)
        gr = ctx.marginal_gemm_stats()
    finally:
        ctx.close()
    assert ev[1] > 0 and ev[1] == gr[1]


@pytest.mark.gpu
def test_arguments_and_states(capi):
    pb, pr, mus, _ = _pair_case(15, 12, "base")
    ctx = capi.Context(pb)
    try:
        gm = _params(pb, CONFIGS["gamma_err_rho_0.25"])       # K = 3 on a context made for one category, and no error model
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.expected_events(gm)
        bad = type(pr)(lambdas=np.array([-0.01, 0.006]), prior=pr.prior)
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.expected_events(bad)
        before = ctx.score(pr)
        ctx.expected_events(pr)
        assert ctx.score(pr) == before                       # a later cafe_score is unaffected
        ctx.comm_attach(capi.comm_unique_id(), 1, 0)
        with pytest.raises(capi.CafeError, match="code 4"):   # CAFE_ERR_STATE
            ctx.expected_events(pr)
        ctx.comm_detach()
    finally:
        ctx.close()
