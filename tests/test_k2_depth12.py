"""K2 (prune_gemm.hip) with 12-deep K tiles, and its per-k-step row-block masks.

The sum over k runs in the same ascending 4-deep k-steps at every depth of a K tile (8, 12, 16), and an MFMA that the masks
leave out would have added exact zeros, so every result has the same bits whatever the depth and whether or not anything is
skipped.  What differs is the staging: a [12][rows] A image is no whole number of 1 KB pieces, a K tile has an odd number of
k-steps (the B fragment pairs alternate across K tiles), the last K tile may stage rows past round_up(M + 1, 16), and a
12-deep K tile overhangs a panel extent rounded to 16 rows -- the rows an assemble pass leaves unwritten.

The rule the kernel's masks and cafe_executed_flops follow, counted independently below: row block b (16 parent sizes) of an
op issues its two MFMAs per wave in k-step s (k = 4s .. 4s + 3) of a column tile exactly when s lies in
[max(a_lo, p_lo) / 4, min(a_hi, p_hi, M) / 4], where [a_lo, a_hi] is the block's matrix extent and [p_lo, p_hi] the panel
extent of the column tile ([0, 0] when that is empty); nothing when the range is empty.  Flops count the valid k (<= M) and
the valid rows only.  Tile height and K-tile depth do not enter."""
import os

import numpy as np
import pytest

from cafexp_amd import problem as P, synth
from helpers import rel_err

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-10
NEWICK = "(((A:1,B:2):1,C:1.5):0.7,((D:1,E:1):2,(F:0.5,(G:1,H:3):1):1):1);"


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _context(capi, pb, max_categories, **env):
    """A context created under the given environment switches (they are read at cafe_create only)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.Context(pb, max_categories=max_categories)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _random_problem(rng, n_fam, M, R, hi):
    tree = P.parse_newick(NEWICK)
    names = [l.name for l in tree.leaves()]
    counts = rng.integers(0, hi, size=(n_fam, len(names))).astype(np.int32)
    return P.build_problem(tree, names, ["f%d" % i for i in range(n_fam)], counts, root_filter=False,
                           max_family_size=M, max_root_family_size=R)


def _same_bits(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert a[1].keys() == b[1].keys()
    for key in a[1]:
        assert np.array_equal(a[1][key], b[1][key]), (what, key)


# (50, 30): 51 mod 12 = 3, one k-step in the last K tile; (59, 40): a full last K tile; (70, 75): 71 mod 12 = 11, three
# k-steps, root rows > M; (60, 30) and (76, 60): 61 = 13 and 77 = 29 mod 48, rounding to 12 exceeds rounding to 16;
# (135, 140): several row tiles at every height
@pytest.mark.parametrize("M,R", [(50, 30), (59, 40), (70, 75), (60, 30), (76, 60), (135, 140)])
def test_every_row_tile_height_at_depth_12(capi, oracle, M, R):
    rng = np.random.default_rng(M * 1000 + R)
    pb = _random_problem(rng, 150, M, R, min(M - 10, 40))
    probs, mult = oracle.discrete_gamma(2, 1.1)
    prs = (P.Params(lambdas=np.array([0.015]), prior=P.prior_uniform(R)),
           P.Params(lambdas=np.array([0.015]), prior=P.prior_uniform(R), multipliers=mult, cat_probs=probs))
    wants = [oracle.score(pb, pr) for pr in prs]
    c8 = _context(capi, pb, 2, CAFE_KB="8")
    ref = [c8.score(pr, alpha=1.1, per_family=True) for pr in prs]
    c12 = _context(capi, pb, 2, CAFE_KB="12")
    for mi in (0, 2, 3, 4, 5, 6, 7, 8, 9):
        c12.force_tile(mi)
        for pr, want, r8 in zip(prs, wants, ref):
            got = c12.score(pr, alpha=1.1, per_family=True)
            assert rel_err(got[0], want) <= SCORE_TOL, (M, R, mi, got[0], want)
            _same_bits(got, r8, (M, R, mi))
    c8.close()
    c12.close()


def _count_issued_flops(ctx, pb, K):
    """The rule of the module docstring, from cafe_get_extents alone."""
    M, R = pb.max_family_size, pb.max_root_family_size
    root = int(np.nonzero(np.asarray(pb.parent) < 0)[0][0])
    total = 0
    for v in range(pb.n_nodes):
        if pb.leaf_taxon[v] >= 0 or v == root:
            continue
        rows = R if pb.parent[v] == root else M
        for k in range(K):
            m, pt = ctx.extents(v, k)
            assert pt is not None
            p_lo, p_hi = pt[:, 0].astype(np.int64), pt[:, 1].astype(np.int64)
            empty = p_hi < p_lo
            p_lo, p_hi = np.where(empty, 0, p_lo), np.where(empty, 0, np.minimum(p_hi, M))
            for b in range(len(m)):
                if 16 * b >= rows:
                    break
                lo, hi = np.maximum(m[b, 0], p_lo), np.minimum(m[b, 1], p_hi)
                live = hi >= lo
                kk = np.minimum((hi // 4 - lo // 4 + 1) * 4, M + 1 - lo // 4 * 4)
                total += 2 * min(16, rows - 16 * b) * int(kk[live].sum()) * 128
    return total


@pytest.fixture(scope="module")
def extent_problem(oracle):
    pb, _ = synth.make_problem(n_taxa=16, n_families=1500, max_count=250, lam_sim=0.003, seed=11, root_cap=120)
    assert pb.matrix_size >= 256                             # (below that the library does not bother with extents)
    probs, mult = oracle.discrete_gamma(3, 1.1)
    # wide, narrow, wide extents on one context: all-zero tiles, one-K-tile ranges, rows left over from the previous call
    calls = [P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(pb.max_root_family_size), multipliers=mult, cat_probs=probs)
             for lam in (0.003, 0.0004, 0.003)]
    return pb, calls


def _three_calls(ctx, calls, count_with=None):
    out, flops = [], []
    for pr in calls:
        out.append(ctx.score(pr, alpha=1.1, per_family=True))
        if count_with is not None:
            flops.append((ctx.executed_flops(), ctx.stats()["gemm_flops"], _count_issued_flops(ctx, count_with, 3)))
    return out, flops


def test_skipping_at_depth_12_changes_no_bit_and_is_counted(capi, extent_problem):
    pb, calls = extent_problem
    c12 = _context(capi, pb, 3, CAFE_KB="12")
    c12.set_profiling(True)                                  # (a launch list for executed_flops)
    got12, flops12 = _three_calls(c12, calls, pb)
    c8 = _context(capi, pb, 3, CAFE_KB="8")
    c8.set_profiling(True)
    got8, flops8 = _three_calls(c8, calls, pb)
    full = _context(capi, pb, 3, CAFE_KB="12", CAFE_NO_KSKIP="1")
    full.set_profiling(True)
    got_full = []
    for pr in calls:
        got_full.append(full.score(pr, alpha=1.1, per_family=True))
        assert full.executed_flops() == full.stats()["gemm_flops"]
    for i in range(3):
        _same_bits(got12[i], got8[i], ("depth 8", i))
        _same_bits(got12[i], got_full[i], ("no skipping", i))
        for executed, dense, counted in (flops12[i], flops8[i]):
            print("call %d: executed %.6e of %.6e, counted %.6e" % (i, executed, dense, counted))
            assert 0 < executed < dense
            assert executed == counted
        assert flops12[i][0] == flops8[i][0]                 # the MFMAs issued do not depend on the depth of a K tile
    assert got12[0][0] == got12[2][0] and got12[0][0] != got12[1][0]
    for c in (c8, c12, full):
        c.close()


@pytest.mark.parametrize("mi", [2, 3, 4, 5])
def test_skipping_at_depth_12_at_forced_heights(capi, extent_problem, mi):
    pb, calls = extent_problem
    full = _context(capi, pb, 3, CAFE_KB="12", CAFE_NO_KSKIP="1")
    c12 = _context(capi, pb, 3, CAFE_KB="12")
    c8 = _context(capi, pb, 3, CAFE_KB="8")
    for c in (c12, c8):
        c.force_tile(mi)
    want, _ = _three_calls(full, calls)
    got12, _ = _three_calls(c12, calls)
    got8, _ = _three_calls(c8, calls)
    for i in range(3):
        _same_bits(got12[i], want[i], ("depth 12", mi, i))
        _same_bits(got8[i], want[i], ("depth 8", mi, i))
    for c in (c8, c12, full):
        c.close()
