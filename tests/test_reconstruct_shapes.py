"""cafe_reconstruct and cafe_branch_probabilities (csrc/reconstruct.hip) away from the workload shapes of test_reconstruct.py:
every edge of K5's row groups (a wave's 16 parent sizes, 64 per block), of the groups of four child sizes and the clamped
look-ahead, of K1's extents per 16 parent sizes, of the row-group flags and their switch-off above 64 groups (M > 1024), of
the four-segment scan on the way down, and of the XCD-aware decoding of the grid into column tiles.

The states are compared for EQUALITY, ties included, every family of every case.  Every value the kernels compare is a chain
of single fp64 multiplies and max -- no addition, hence no FMA contraction and no summation order -- so the numpy statement
(tests/joint_ref.py), multiplying in the same association on the matrices the device itself built, produces the same bits.
tests/test_reconstruct_model.py shows on the CPU that this statement is the oracle's, that the pairs reach the edges, that
the inputs put states on the guards, and that each of eight wrong statements is told apart by these inputs.

cafe_create publishes K1's extents from matrix order 256 on: below it K5 and the way down run without them, so the extent
edges are those of the six pairs from (255, 256) up and of the two variant cases at (255, 256).

cafe_reconstruct leaves nothing to read back (cafe_get_matrix answers CAFE_ERR_STATE after it), so the matrices are read after
a cafe_root_max at the same rates -- per gamma category at lambda * multiplier, the product the library itself forms: the
same key through the same builder, hence the bits cafe_reconstruct worked on.

Viterbi sums: NaN masks identical, values to 1e-12 relative -- both sums run left to right over at most 2048 non-negative
terms, each partial sum within M 2^-53 <= 2.3e-13 of the exact one.
"""
import numpy as np
import pytest

import joint_ref as JR
import marginal_ref as MR
from bd_lm_ref import MUS
from test_marginal_shapes import SWEEP_LAMBDA, SWEEP_TREE
from test_reconstruct import _check_bp
from test_reconstruct_model import (DUPLICATED_ROW, PAIRS, SATURATED, VARIANTS, double_families, flags_path, interior, node, root_prior,
                                    sweep_case, variant_case, viterbi_sizes)

pytestmark = pytest.mark.gpu

DEATH_RATE = MUS[:1]                                         # one lambda class in the sweep: tests/bd_lm_ref.py's first death rate


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _context(capi, case, pb=None, **kw):
    ctx = capi.Context(case.pb if pb is None else pb, max_categories=case.K, **kw)
    if case.mus is not None:
        ctx.set_death_rates(case.mus)
    return ctx


def _device_matrices(ctx, case, pb=None):
    """mats[k][v] as this context builds them at the case's rates (module docstring)"""
    pb = case.pb if pb is None else pb
    mults = [1.0] if case.multipliers is None else list(case.multipliers)
    out = []
    for m in mults:
        ctx.root_max(case.lambdas * m)
        out.append(MR.context_matrices(ctx, pb, 1)[0])
    return out


def _equal_to_numpy(got, case, mats, label):
    """got [K][F][n] against joint_ref, every family and node; returns the reference's (states, info) per category"""
    pb = case.pb
    assert got.shape == (case.K, pb.n_families, pb.n_nodes)
    leaves = np.where(pb.leaf_taxon >= 0)[0]
    refs = []
    for k in range(case.K):
        want, info = JR.joint_reconstruct(pb, case.rp, mats[k])
        bad = np.nonzero((got[k] != want).any(axis=1))[0]
        assert len(bad) == 0, "%s category %d: families %s differ, first: device %s numpy %s" % (label, k, bad.tolist(), got[k][bad[0]], want[bad[0]])
        assert np.array_equal(got[k][:, leaves], pb.counts[:, pb.leaf_taxon[leaves]])
        assert np.array_equal(got[k][7], got[k][DUPLICATED_ROW])
        refs.append((want, info))
    return refs


def _run(capi, case, label, monkeypatch=None):
    """One context: reconstruct, the matrices, reconstruct again (the calls between change nothing), the comparison; with
    monkeypatch also a context whose row-group flags are switched off.  Returns (context, device states, references)."""
    ctx = _context(capi, case)
    got = ctx.reconstruct(case.lambdas, case.rp, multipliers=case.multipliers)
    mats = _device_matrices(ctx, case)
    assert np.array_equal(ctx.reconstruct(case.lambdas, case.rp, multipliers=case.multipliers), got)
    refs = _equal_to_numpy(got, case, mats, label)
    if monkeypatch is not None:
        monkeypatch.setenv("CAFE_NO_RECON_FLAGS", "1")
        plain = _context(capi, case)
        try:
            assert np.array_equal(plain.reconstruct(case.lambdas, case.rp, multipliers=case.multipliers), got)
        finally:
            plain.close()
            monkeypatch.delenv("CAFE_NO_RECON_FLAGS")
    return ctx, got, refs


@pytest.mark.parametrize("M,R", PAIRS)
def test_sweep_of_row_groups_and_extents(capi, monkeypatch, M, R):
    case = sweep_case(M, R)
    pb = case.pb
    ctx, got, refs = _run(capi, case, "sweep M %d R %d" % (M, R), monkeypatch if flags_path(M) else None)
    try:
        print("M %d R %d: %s" % (M, R, "row-group flags" if flags_path(M) else "flags off (more than 64 row groups)"))
        want, info = refs[0]
        inner = interior(pb)
        if M > 16:
            assert (want[:, inner] > 16 * ((M - 1) // 16)).any()         # the last row group is visited
        assert (want == M).any() and (want == 0).any() and np.all(info["root_value"] > 0)
        assert np.isfinite(ctx.score(case.params()))                     # the scorer path on the same context afterwards
    finally:
        ctx.close()


@pytest.mark.parametrize("name", VARIANTS)
def test_variant_cases(capi, monkeypatch, name):
    """(33, 20): a saturated interior branch (all-zero rows, children through row 0), two lambdas, three gamma categories.
    (255, 256), where the context has K1's extents: the saturated branch again -- an empty extent, K5 walks nothing and the
    way down scans nothing -- and pure birth, the one input on which backtrack_kernel's start value behind an extent with
    lo > 0 decides a state."""
    case = variant_case(name)
    ctx, got, refs = _run(capi, case, name, monkeypatch)
    try:
        abcd = node(case.pb, "A", "B", "C", "D")
        if case.pb.matrix_size >= 256:
            ctx.root_max(case.lambdas)
            lo, hi = (int(x) for x in ctx.extents(abcd)[0][0])           # K1's extent of parent sizes 1..16 on the branch above ((A,B),(C,D))
    finally:
        ctx.close()
    zero_rows = sum(int(info["zero_row"].sum()) for _, info in refs)
    via_row0 = sum(int(info["via_row0"].sum()) for _, info in refs)
    if name in SATURATED:
        assert zero_rows > 0 and via_row0 > 0
    if name == "saturated_with_extents":
        assert hi < lo                                       # an empty extent
    if name == "pure_birth":
        assert zero_rows > 0 and (refs[0][0][:, abcd] == 0).any() and 1 <= lo <= hi      # scanned from lo >= 1, and 0 is the answer


@pytest.mark.parametrize("M,R", [(33, 20), (129, 130), (255, 256)])         # the last one with K1's extents
def test_sweep_under_death_rates(capi, monkeypatch, M, R):
    case = sweep_case(M, R, mus=DEATH_RATE)
    ctx, got, refs = _run(capi, case, "death rates M %d R %d" % (M, R), monkeypatch)
    ctx.close()
    plain = sweep_case(M, R)
    ctx, other, _ = _run(capi, plain, "equal rates M %d R %d" % (M, R))
    ctx.close()
    assert not np.array_equal(got, other)                    # the death rate reached the matrices of this path


def test_column_tiles_of_distinct_families(capi):
    """1100 distinct families at M = 33: 1152 columns, 18 tiles of 64 -- K5's grid decoding ct = xcd + 8 (slot / n_rg) takes a
    third round and the blocks of tiles 18..23 return early; and the same through single 128-column chunks."""
    M, R = 33, 20
    rng = np.random.default_rng(33)
    rows = np.unique(rng.integers(0, M + 1, size=(1400, 8)), axis=0)
    rows = rows[rng.permutation(len(rows))[:1100]]
    assert len(rows) == 1100
    from helpers import _explicit_problem
    pb = _explicit_problem(SWEEP_TREE, [dict(zip("ABCDEFGH", map(int, r))) for r in rows], M, R)
    lam, rp = np.array([SWEEP_LAMBDA]), root_prior(M, R)
    whole = capi.Context(pb)
    assert whole.stats()["n_unique_families"] == 1100 > 512
    got = whole.reconstruct(lam, rp)[0]
    whole.root_max(lam)
    want, _ = JR.joint_reconstruct(pb, rp, MR.context_matrices(whole, pb, 1)[0])
    whole.close()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (bad.tolist(), got[bad[0]], want[bad[0]])
    n_interior = len(interior(pb))
    rows4 = (M + 1 + 3) // 4 * 4
    small = capi.Context(pb, workspace_limit=(n_interior * rows4 * 8 + 2 * pb.n_nodes * 4 + n_interior * 4 + 1) * 128 + 64)
    assert np.array_equal(small.reconstruct(lam, rp)[0], got)
    small.close()


@pytest.mark.parametrize("M,R,two_rates", [(2, 2, False), (16, 16, False), (33, 20, False), (33, 20, True), (129, 130, False), (1025, 1100, False)])
def test_branch_probabilities(capi, M, R, two_rates):
    """viterbi_kernel: the reconstructed states and seeded rows with a parent at 0, a child at M, a parent at M and parent ==
    child, on a leaf branch (row-major matrix) and on an interior branch (k-major matrix)."""
    case = sweep_case(M, R, mus=DEATH_RATE if two_rates else None)
    pb2 = double_families(case.pb)
    ctx = _context(capi, case, pb=pb2)
    try:
        states = ctx.reconstruct(case.lambdas, case.rp)[0][:case.pb.n_families]
        mats = _device_matrices(ctx, case, pb=pb2)[0]
        assert np.array_equal(states, JR.joint_reconstruct(case.pb, case.rp, mats)[0])
        sizes = viterbi_sizes(case.pb, states, seed=M)
        got = ctx.branch_probabilities(case.lambdas, sizes)
    finally:
        ctx.close()
    want = JR.branch_probabilities(pb2, sizes, mats)
    root = MR.root_of(pb2)
    par = pb2.parent
    invalid = np.array([[v == root or sizes[f, v] == sizes[f, par[v]] for v in range(pb2.n_nodes)] for f in range(len(sizes))])
    assert np.array_equal(np.isnan(want), invalid) and (~invalid).sum() > len(sizes)
    _check_bp(got, want, 1e-12)
