"""cafe_leaf_predictive (csrc/predictive.hip) at the smallest shapes at which each of its kernels can go wrong: the inputs of
tests/test_gradient_shapes.py, with the counts of its random families brought within reach of each other (_tamed) where a
single category leaves sd's cancellation above the constant of the bound.

Tree: a cherry, a polytomy of 7 leaves (a leaf's six siblings fill one product launch), a leaf beside an interior sibling and
leaf M under the root, whose GEMM contracts over the root's sizes 0..R; two lambda classes.  (M, R) in PAIRS: M + 1, the GEMM's
output rows, on either side of its 64-row tile, and the contraction length (M + 1, or R + 1 under the root) on either side of the
16-deep K step, with R below and above M.  Families: counts 0 and M at leaves under a 3-tap error model (taps fall outside
[0, M]), every leaf at M, duplicates.  Models (CONFIGS of that file): base with lambda = mu; gamma K = 3 with the error model and
death rates four times the lambdas; base with the error model and death rates a quarter of them.  Column counts 1, 127, 128, 129
and 300 distinct families, as that file draws them (the gamma configuration's three categories keep their factor below 100); a
table whose families have leaves at 0 or at M under gamma x error model x death rates.

Reference and bound: leaf_predictive_ref.reference on numpy matrices, |got - ref| <= 1e-12 + 1e-10 c |ref| with c = C_BOUND for sd
(each cell held to its own factor 1 + (mean - x)^2 / var, at most C_BOUND) and 1 for the sums of non-negative terms;
tests/test_leaf_predictive_model.py measures the factors of these inputs on the CPU.

Bits: three column batches against one; duplicated families; and one species' counts permuted among the families, which must
leave that species' mean and sd of every family as they were -- they are functions of the other species' counts alone."""
import functools

import numpy as np
import pytest

import leaf_predictive_ref as LR
from test_gradient_shapes import COLUMNS, CONFIGS, PAIRS, SPECIES, _K, _params, _problem, kBN

C_BOUND = 100.0                                              # the cap on a cell's own factor (test_leaf_predictive_model measures them)


def _tamed(pb):
    """_problem's table with the counts of a family brought within reach of each other.  Its random rows draw every species
    from 0..12 on its own, which no rate of CONFIGS makes likely: the base configurations put such cells 10 to 22 sd from their
    prediction, and sd's factor 1 + (mean - x)^2 / var reaches 487 (test_leaf_predictive_model has the figures, and those of the
    rates tried).  A family whose counts span more than 2 gets its first species' count, at least 3, plus -1, 0 or 1 (its own
    count mod 3) in every species -- at a base of 0 or 1 six siblings at 0 leave a leaf's prediction no width at all -- and
    species M, which hangs under the root, gets at most R, the root's largest size.  The rows _problem sets by hand (all 1,
    all M, M - 2..M, 0..2, the duplicates) span at most 2 and stay as they are but for that last rule."""
    M, R = pb.max_family_size, pb.max_root_family_size
    counts = pb.counts.copy()
    wide = counts.max(axis=1) - counts.min(axis=1) > 2
    counts[wide] = np.clip(np.maximum(counts[wide][:, :1], 3) + counts[wide] % 3 - 1, 0, M)
    counts[:, SPECIES.index("M")] = np.minimum(counts[:, SPECIES.index("M")], R)
    pb.counts = np.ascontiguousarray(counts.astype(np.int32))
    return pb


def _with_ref(pb, pr, mus):
    return pb, pr, mus, LR.reference(pb, pr, LR.matrices(pb, pr, mus))


@functools.lru_cache(maxsize=None)
def _pair_case(M, R, config):
    cfg = CONFIGS[config]
    pb = _tamed(_problem(M, R, err=cfg["err"]))
    return _with_ref(pb, _params(pb, cfg), cfg["mus"])


@functools.lru_cache(maxsize=None)
def _column_case(n):
    cfg = CONFIGS["gamma_err_rho_0.25"]
    pb = _problem(40, 30, n=n, seed=n, err=True, distinct=True)
    return _with_ref(pb, _params(pb, cfg), cfg["mus"])


@functools.lru_cache(maxsize=None)
def _edge_case():
    """every other family has its leaves at 0 and 1 with species A at 0 (the lower tap falls outside), the rest at M - 1 and M
    with species A at M (the upper one does); a family with leaves at both ends has cells 20 sd from their prediction"""
    M, R = 20, 16
    cfg = CONFIGS["gamma_err_rho_0.25"]
    pb = _problem(M, R, err=True)
    rng = np.random.default_rng(5)
    high = (np.arange(pb.n_families) % 2 == 1)[:, None]
    counts = np.where(high, M - 1, 0) + rng.integers(0, 2, size=pb.counts.shape)
    counts[:, 0] = np.where(high[:, 0], M, 0)
    counts[:, 12] = np.minimum(counts[:, 12], R)             # species M hangs under the root, whose sizes end at R
    pb.counts = np.ascontiguousarray(counts.astype(np.int32))
    return _with_ref(pb, _params(pb, cfg), cfg["mus"])


@functools.lru_cache(maxsize=None)
def _permuted_case(species):
    """the 300 distinct families with one species' counts rotated by 7 families"""
    pb, pr, mus, _ = _column_case(300)
    t = SPECIES.index(species)
    counts = pb.counts.copy()
    counts[:, t] = np.roll(counts[:, t], 7)
    other = _problem(40, 30, n=300, seed=300, err=True, distinct=True)
    other.counts = np.ascontiguousarray(counts)
    return other, t


def input_sets():
    """every (label, case) the GPU tests of this file run: what the CPU tests measure"""
    for M, R in PAIRS:
        for config in sorted(CONFIGS):
            yield "M %d R %d %s" % (M, R, config), _pair_case(M, R, config)
    for n in COLUMNS:
        yield "%d distinct families" % n, _column_case(n)
    yield "taps at 0 and M", _edge_case()


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _run(capi, pb, pr, mus, ref=None, label="", marginal=False, **ctx_args):
    ctx = capi.Context(pb, max_categories=_K(pr), **ctx_args)
    try:
        ctx.set_death_rates(mus)
        got = ctx.leaf_predictive(pr, alpha=0.7)
        if marginal:
            got["marginal_log_evidence"] = ctx.marginal_reconstruct(pr, alpha=0.7)["log_evidence"]
    finally:
        ctx.close()
    if ref is not None:
        LR.close(got, ref, C_BOUND, label)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("M,R", PAIRS)
def test_every_pair_and_model(capi, M, R, config):
    pb, pr, mus, ref = _pair_case(M, R, config)
    got = _run(capi, pb, pr, mus, ref, "M %d R %d %s" % (M, R, config))
    assert not got["failed"].any() and not np.isnan(got["mean"]).any()
    total = got["p_below"] + got["p_obs"] + got["p_above"]
    assert np.all(np.abs(total - 1.0) <= 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("n", COLUMNS)
def test_column_counts_around_the_tile(capi, n):
    pb, pr, mus, ref = _column_case(n)
    assert len(np.unique(pb.counts, axis=0)) == n
    _run(capi, pb, pr, mus, ref, "%d distinct families" % n)


@pytest.mark.gpu
def test_taps_at_zero_and_at_the_largest_size(capi):
    pb, pr, mus, ref = _edge_case()
    assert pr.error_model is not None and pr.multipliers is not None and mus is not None
    assert np.all((pb.counts == 0).any(axis=1) | (pb.counts == pb.max_family_size).any(axis=1))
    assert (pb.counts == 0).any(axis=1).sum() == (pb.counts == pb.max_family_size).any(axis=1).sum() == pb.n_families // 2
    got = _run(capi, pb, pr, mus, ref, "taps at 0 and M")
    at0, atM = pb.counts == 0, pb.counts == pb.max_family_size
    assert np.all(got["p_below"][at0] == 0.0) and np.all(got["p_above"][atM] == 0.0)


def _per_col(pb, K):
    """leaf_predictive_impl's own workspace formula: bytes per column"""
    nI, nL = int((pb.leaf_taxon < 0).sum()), int((pb.leaf_taxon >= 0).sum())
    rows = pb.matrix_size
    return (3 * nI * rows + 3 * rows + K + 6 * nL + 2) * 8


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
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_duplicated_families_get_the_same_bits(capi, config):
    pb, pr, mus, ref = _pair_case(65, 80, config)
    assert np.array_equal(pb.counts[4], pb.counts[2]) and np.array_equal(pb.counts[5], pb.counts[0])
    got = _run(capi, pb, pr, mus)
    for key in LR.KEYS + ("log_evidence",):
        assert np.array_equal(got[key][4], got[key][2], equal_nan=True) and np.array_equal(got[key][5], got[key][0], equal_nan=True), key


@pytest.mark.gpu
@pytest.mark.parametrize("species", ["D", "L", "M"])         # in the polytomy, beside an interior sibling, under the root
def test_a_species_own_counts_do_not_reach_its_mean_and_sd(capi, species):
    pb, pr, mus, ref = _column_case(300)
    other, t = _permuted_case(species)
    assert (other.counts[:, t] != pb.counts[:, t]).mean() > 0.5 and np.array_equal(np.delete(other.counts, t, axis=1), np.delete(pb.counts, t, axis=1))
    want = _run(capi, pb, pr, mus, ref, "as observed")
    got = _run(capi, other, pr, mus)
    for key in ("mean", "sd"):
        assert np.array_equal(got[key][:, t], want[key][:, t]), key
    moved = other.counts[:, t] != pb.counts[:, t]
    assert np.any(got["p_obs"][moved, t] != want["p_obs"][moved, t])


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_observed_count_carries_the_evidence(capi, config):
    """w[x] = Z: log p_obs + log W = log_evidence for every cell.  W is recovered in the reference alone; the device's p_obs is
    compared with the reference's and its log_evidence with cafe_marginal_reconstruct's on the same context."""
    pb, pr, mus, ref = _pair_case(64, 129, config)
    with np.errstate(divide="ignore"):
        lhs = np.log(ref["p_obs"]) + np.log(ref["W"])
    want = np.repeat(ref["log_evidence"][:, None], lhs.shape[1], axis=1)
    assert np.all(np.abs(lhs - want) <= 1e-12 + 1e-10 * np.abs(want))
    got = _run(capi, pb, pr, mus, ref, "identity " + config, marginal=True)
    ml = got["marginal_log_evidence"]
    worst = float(np.max(np.abs(got["log_evidence"] - ml) / (1e-12 + 1e-10 * np.abs(ml))))
    print("%s: worst |log_evidence - cafe_marginal_reconstruct's| / bound %.3g" % (config, worst))
    assert worst <= 1.0
    assert np.all(np.abs(got["p_obs"] - ref["p_obs"]) <= 1e-12 + 1e-10 * np.abs(ref["p_obs"]))
