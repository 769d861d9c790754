"""The passes in front of the prune (extents.hip): the magnitude tables of a call's matrices (mag_tables_kernel), the
intervals and bounds of the panels, one launch per tree level (node_level_kernel), and the K ranges (range_kernel).

The problems are those of tests/test_magnitude_skip.py (_problem): 7 taxa, lam_sim 0.003, a gamma call with K = 2,
lambda = 0.002, alpha = 0.9.  max_count 205 gives matrix order 257, whose 52 row steps are less than a wave; max_count 600
gives order 751, 181 row steps: two full waves and a part of a third.  260 families give three column tiles at the leaves, a
partly filled last tile and de-duplicated columns with inner_map; a table of 100 families gives one tile.

Run as a script (`python tests/test_prepass_tables.py record`) the file prints the issued flops of the four calls of the last
test as JSON: tests/golden/prepass_parent_issued_flops.json is that output for the commit before the level kernel.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path and __name__ == "__main__":
    sys.path.insert(0, ROOT)

from cafexp_amd import problem as P, synth  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("CAFE_NO_MAGSKIP", "CAFE_NO_KSKIP", "CAFE_NO_GROUPS")
ORDERS = {257: 205, 751: 600}            # matrix order -> max_count
MAG_NONE, MAG_UNIT = -(1 << 28), 256
GOLDEN = os.path.join(ROOT, "tests", "golden", "prepass_parent_issued_flops.json")


def _problem(max_count, n_families=260, n_deviations=0, n_taxa=7, seed=5):
    pb, _ = synth.make_problem(n_taxa=n_taxa, n_families=n_families, max_count=max_count, lam_sim=0.003, seed=seed,
                               root_cap=max_count // 2, n_deviations=n_deviations)
    return pb


def _context(capi, pb, env=()):
    saved = {name: os.environ.pop(name, None) for name in SWITCHES}
    try:
        for name in env:
            os.environ[name] = "1"
        return capi.Context(pb, max_categories=2)
    finally:
        for name in SWITCHES:
            os.environ.pop(name, None)
            if saved[name] is not None:
                os.environ[name] = saved[name]


def _params(oracle, pb, lam, gamma, em=None):
    prior = P.prior_uniform(pb.max_root_family_size)
    lambdas = np.full(pb.n_lambdas, lam)
    if not gamma:
        return P.Params(lambdas=lambdas, prior=prior, error_model=em)
    probs, mult = oracle.discrete_gamma(2, 0.9)
    return P.Params(lambdas=lambdas, prior=prior, multipliers=mult, cat_probs=probs, error_model=em)


def _interior_non_root(pb):
    return [v for v in range(len(pb.parent)) if pb.leaf_taxon[v] < 0 and pb.parent[v] >= 0]


def _leaves(pb):
    return [v for v in range(len(pb.parent)) if pb.leaf_taxon[v] >= 0]


def _issued_flops(capi, oracle):
    """{"<order>/<call>": issued flops} of the gamma call and the base call (lambda 0.0015) at both orders, 260 families."""
    out = {}
    for order, max_count in ORDERS.items():
        pb = _problem(max_count)
        ctx = _context(capi, pb)
        for name, pr, alpha in (("gamma", _params(oracle, pb, 0.002, True), 0.9), ("base", _params(oracle, pb, 0.0015, False), 1.0)):
            ctx.score(pr, alpha=alpha)
            out["%d/%s" % (order, name)] = ctx.issued_flops()
        ctx.close()
    return out


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


@pytest.fixture(scope="module")
def scored(capi, oracle):
    """(problem, default context after the gamma call) per (order, families): computed once, read by every test."""
    out = {}
    for order, max_count in ORDERS.items():
        for nf in (260, 100):
            pb = _problem(max_count, n_families=nf)
            assert pb.matrix_size == order
            ctx = _context(capi, pb)
            assert np.isfinite(ctx.score(_params(oracle, pb, 0.002, True), alpha=0.9))
            out[order, nf] = (pb, ctx)
    yield out
    for _, ctx in out.values():
        ctx.close()


def _log2_units(m):
    """256 log2(m) where m > 0, -inf where m == 0"""
    with np.errstate(divide="ignore"):
        return MAG_UNIT * np.log2(m)


def _check_table(got, want_max, what):
    """got: a table as the device wrote it; want_max: the maximum every entry stands for, from the device's own matrix.

    mag_of(v) writes e 256 + ceilf(log2f((float)m) 256) + 1 for v = m 2^e, m in [0.5, 1).  Against x = 256 log2(v) the
    float path is off by at most 256 (2^-24 log2(e) of the conversion of m + 2^-23 of log2f) + 2^-16 of the product, under
    2^-13; ceilf adds less than 1 and the + 1 adds 1.  So   x + 1 - 2^-13 <= entry < x + 2 + 2^-13:   every entry is at
    least log2 of its maximum, without tolerance, and overshoots it by less than 2 + 2^-10 units of 1/256 (the figure
    asserted: the derivation's 2^-13 with room for the double log2 of this check)."""
    assert got.shape == want_max.shape, (what, got.shape, want_max.shape)
    zero = want_max == 0
    assert (got[zero] == MAG_NONE).all(), what
    assert (got[~zero] != MAG_NONE).all(), what
    x = _log2_units(want_max[~zero])
    over = got[~zero].astype(np.float64) - x
    print(what, "entries", int((~zero).sum()), "zero", int(zero.sum()), "overshoot min %.4f max %.4f" % (over.min(), over.max()))
    assert (over >= 0).all(), (what, over.min())
    assert (over < 2 + 2.0 ** -10).all(), (what, over.max())
    return int((~zero).sum()), int(zero.sum())


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_tables_dominate_the_matrices_and_overshoot_by_less_than_two_units(scored, order):
    """Per slot, with P = ctx.matrix(v, k) (the device's matrix): a16[ks][b] stands for the largest P[s][c], s in
    16 b + 1 .. 16 b + 16, c in 4 ks .. 4 ks + 3; t4[ks][r] for the largest row sum over those four c (added in the
    kernel's order) for s in 4 r .. 4 r + 3, the size-0 row being e_0; lt[x][r] for the largest P[s][x], s in 4 r .. 4 r + 3.
    Every entry is >= 256 log2 of its maximum and less than 2 + 2^-10 units above it (_check_table has the derivation);
    where the maximum is zero the table says kMagNone, and nowhere else."""
    pb, ctx = scored[order, 260]
    n, M = pb.matrix_size, pb.max_family_size
    nk, nr, nb = (M + 1 + 3) // 4, (n + 3) // 4, (n - 1 + 15) // 16
    rows = max(4 * nr, 16 * nb + 1)
    live = none = 0
    for k in range(2):
        for v in _interior_non_root(pb):
            Pm = ctx.matrix(v, k)
            pad = np.zeros((rows, 4 * nk))
            pad[:n, :M + 1] = Pm[:, :M + 1]
            sum4 = ((pad[:, 0::4] + pad[:, 1::4]) + pad[:, 2::4]) + pad[:, 3::4]
            max4 = pad.reshape(rows, nk, 4).max(axis=2)
            a, b = _check_table(ctx.magnitude_tables("t4", v, k), sum4[:4 * nr].reshape(nr, 4, nk).max(axis=1).T, ("t4", order, v, k))
            live += a; none += b
            a, b = _check_table(ctx.magnitude_tables("a16", v, k), max4[1:16 * nb + 1].reshape(nb, 16, nk).max(axis=1).T, ("a16", order, v, k))
            live += a; none += b
        for v in _leaves(pb):
            Pm = ctx.matrix(v, k)
            pad = np.zeros((4 * nr, M + 1))
            pad[:n] = Pm[:, :M + 1]
            want = pad.reshape(nr, 4, M + 1).max(axis=1).T
            want[0, 0] = max(want[0, 0], 1.0)
            a, b = _check_table(ctx.magnitude_tables("lt", v, k), want, ("lt", order, v, k))
            live += a; none += b
    assert live > 10000 and none > 0                         # (both kinds of entry were met)


@pytest.mark.parametrize("families", [260, 100])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_rows_outside_the_hull_say_nothing(scored, order, families):
    """panel_bounds(v, k)[ct, r] is -inf exactly for the row steps outside the hull of column_extents(v, k) over the tile's
    128 columns, and finite and >= -1050 inside: every interior non-root node, both categories."""
    pb, ctx = scored[order, families]
    _check_hulls(pb, ctx, 1 if families == 100 else None)
    if families == 260:
        assert max(len(ctx.column_extents(v, 0)) for v in _interior_non_root(pb)) >= 3 * 128


def _check_hulls(pb, ctx, n_tiles=None):
    inside = outside = 0
    for v in _interior_non_root(pb):
        for k in range(2):
            ext = ctx.column_extents(v, k).astype(np.int64)
            bound = ctx.panel_bounds(v, k)
            assert ext.shape[0] % 128 == 0 and bound.shape[0] == ext.shape[0] // 128
            assert n_tiles is None or bound.shape[0] == n_tiles
            lo = ext[:, 0].reshape(-1, 128).min(axis=1)
            hi = ext[:, 1].reshape(-1, 128).max(axis=1)
            r = np.arange(bound.shape[1])
            live = (hi >= lo)[:, None] & (4 * r[None, :] + 3 >= lo[:, None]) & (4 * r[None, :] <= hi[:, None])
            assert (np.isneginf(bound) == ~live).all(), (v, k)
            assert np.isfinite(bound[live]).all() and (bound[live] >= -1050).all(), (v, k)
            inside += int(live.sum()); outside += int((~live).sum())
    assert inside > 0 and outside > 0


def _all_extents_and_ranges(pb, ctx):
    return {(v, k): (ctx.column_extents(v, k), ctx.k_ranges(v, k).astype(np.int64)) for v in _interior_non_root(pb) for k in range(2)}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_intervals_do_not_depend_on_whether_bounds_are_computed(capi, oracle, scored, order):
    """The level kernel runs the intervals with and without magnitude tables.  column_extents of a default context equal
    those of CAFE_NO_MAGSKIP=1, bit for bit, and every K range lies inside that context's.  With an error model (the 3-tap
    model of test_magnitude_skip) the call keeps no bounds in either context: intervals and ranges are equal and
    issued_flops() == executed_flops()."""
    pb, ctx = scored[order, 260]
    exact = _context(capi, pb, ("CAFE_NO_MAGSKIP",))
    exact.score(_params(oracle, pb, 0.002, True), alpha=0.9)
    new, old = _all_extents_and_ranges(pb, ctx), _all_extents_and_ranges(pb, exact)
    exact.close()
    shorter = 0
    for key in old:
        assert new[key][0].tobytes() == old[key][0].tobytes(), key
        n, o = new[key][1], old[key][1]
        assert n.shape == o.shape
        some, was = n[..., 1] >= n[..., 0], o[..., 1] >= o[..., 0]
        assert not (some & ~was).any(), key
        assert (n[..., 0][some] >= o[..., 0][some]).all() and (n[..., 1][some] <= o[..., 1][some]).all(), key
        shorter += int((np.where(some, n[..., 1] - n[..., 0] + 1, 0) < np.where(was, o[..., 1] - o[..., 0] + 1, 0)).sum())
    assert shorter > 0
    pe = _problem(ORDERS[order], n_deviations=3)
    em = P.error_model_table(P.default_error_model(pe.max_family_size)[:1] + [[0.05, 0.9, 0.05]], pe.max_family_size)
    got = []
    for env in ((), ("CAFE_NO_MAGSKIP",)):
        c = _context(capi, pe, env)
        c.score(_params(oracle, pe, 0.002, True, em), alpha=0.9)
        assert c.issued_flops() == c.executed_flops()
        got.append(_all_extents_and_ranges(pe, c))
        c.close()
    for key in got[0]:
        assert got[0][key][0].tobytes() == got[1][key][0].tobytes(), key
        assert got[0][key][1].tobytes() == got[1][key][1].tobytes(), key


def test_the_bound_did_not_get_looser(capi, oracle):
    """issued_flops() of the gamma call and of the base call (lambda 0.0015) at orders 751 and 257, 260 families, is at most
    what the commit before the level kernel issues for the same call (tests/golden/prepass_parent_issued_flops.json, recorded
    by this file run as a script against that commit's library).  Issued flops are whole numbers in a double: no tolerance."""
    with open(GOLDEN) as f:
        parent = json.load(f)["issued_flops"]
    got = _issued_flops(capi, oracle)
    print("issued flops:", got, "parent:", parent)
    assert sorted(got) == sorted(parent)
    for key, value in got.items():
        assert value <= parent[key], (key, value, parent[key])


def _state(pb, ctx, K):
    """what the passes left behind after a call: intervals, bounds and ranges of every interior non-root node, as bytes"""
    return {(v, k): (ctx.column_extents(v, k).tobytes(), ctx.panel_bounds(v, k).tobytes(), ctx.k_ranges(v, k).tobytes())
            for v in _interior_non_root(pb) for k in range(K)}


@pytest.mark.parametrize("order,families", [(257, 260), (751, 260), (257, 700)])
def test_bounds_do_not_depend_on_the_tiles_a_workgroup_owns(capi, oracle, order, families):
    """The level kernel gives a workgroup 1, 2 or 4 column tiles by the size of the level; the problems of this suite are small
    enough for 1 everywhere, the bench runs 4.  Context.set_level_tiles forces the number.  260 families are three tiles at
    the leaves (a pair and a single tile; three of four), 700 are six (two workgroups of four, the second half filled; the
    nodes above, with fewer columns, other remainders).  Under 2 and 4 tiles per workgroup the rows outside the hulls say
    nothing (as test_rows_outside_the_hull_say_nothing), and intervals, bounds and K ranges of every node, and the issued
    flops of the gamma and the base call, are those of 1 tile per workgroup byte for byte: a tile's k-step sum runs on an
    absolute grid of rounds and meets the same terms in the same order whatever its neighbours are.  So everything the
    magnitude tests pin at 1 tile (domination, the audit of the skipped steps) holds for the bench's 4; the next test checks
    domination at 2 and 4 directly.  At 260 families the flops are also within the parent's recorded ones."""
    pb = _problem(ORDERS[order], n_families=families)
    ctx = _context(capi, pb)
    calls = (("gamma", _params(oracle, pb, 0.002, True), 0.9), ("base", _params(oracle, pb, 0.0015, False), 1.0))
    with open(GOLDEN) as f:
        parent = json.load(f)["issued_flops"]
    got = {}
    for tiles in (1, 2, 4):
        ctx.set_level_tiles(tiles)
        for name, pr, alpha in calls:
            value = ctx.score(pr, alpha=alpha)
            if name == "gamma":
                _check_hulls(pb, ctx)
            got[tiles, name] = (value, ctx.issued_flops(), _state(pb, ctx, 2 if name == "gamma" else 1))
    widest = max(len(ctx.column_extents(v, 0)) for v in _interior_non_root(pb)) // 128
    assert widest >= (5 if families == 700 else 3) and widest % 4 != 0
    for (tiles, name), (value, flops, state) in got.items():
        assert np.float64(value).tobytes() == np.float64(got[1, name][0]).tobytes(), (tiles, name)
        assert flops == got[1, name][1], (tiles, name, flops, got[1, name][1])
        assert state == got[1, name][2], (tiles, name, [key for key in state if state[key] != got[1, name][2][key]][:4])
        if families == 260:
            assert flops <= parent["%d/%s" % (order, name)], (tiles, name)
    ctx.close()


@pytest.mark.parametrize("tiles", [2, 4])
def test_bounds_dominate_the_panels_with_several_tiles_per_workgroup(capi, oracle, tiles):
    """As the bound check of tests/test_magnitude_audit.py, with the level kernel forced to 2 and to 4 tiles per workgroup:
    700 families at order 257 in the order of their largest count, a context without dedup (panel column f is family f, six
    column tiles at every node), panels computed on the CPU from the device's own matrices.  panel_bounds(v, k)[ct, r] >=
    log2 of every entry of rows 4 r .. 4 r + 3 of tile ct, without tolerance, and >= -1060 wherever an entry is not zero."""
    import magskip_ref as R
    pb = _problem(ORDERS[257], n_families=700)
    order = np.argsort(pb.counts.max(axis=1), kind="stable")
    pb = dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[order]), family_ids=[pb.family_ids[i] for i in order])
    F, M = pb.n_families, pb.max_family_size
    n_tiles = (F + 127) // 128
    assert n_tiles == 6
    for name in SWITCHES:
        assert name not in os.environ
    ctx = capi.Context(pb, max_categories=2, dedup=False, subtree_dedup=False)
    ctx.set_level_tiles(tiles)
    assert np.isfinite(ctx.score(_params(oracle, pb, 0.002, True), alpha=0.9))
    checked = 0
    for k in range(2):
        mats = {v: ctx.matrix(v, k) for v in range(pb.n_nodes) if pb.parent[v] >= 0}
        panels = R.cpu_panels(pb, mats, pb.counts)
        for v in R.interior_non_root(pb):
            L, bound = panels[v], ctx.panel_bounds(v, k)
            assert L.shape == (M + 1, F) and bound.shape[0] == n_tiles and bound.shape[1] * 4 >= M + 1
            Lp = np.zeros((4 * bound.shape[1], 128 * n_tiles))
            Lp[:M + 1, :F] = L
            top = R._log2(Lp.reshape(bound.shape[1], 4, n_tiles, 128).max(axis=(1, 3))).T      # [tile][row step]
            assert (bound >= top).all(), (v, k, np.argwhere(bound < top)[:4])
            assert (bound[np.isfinite(top)] >= -1060).all()
            checked += int(np.isfinite(top).sum())
    assert checked > 1000
    ctx.close()


if __name__ == "__main__":
    from cafexp_amd import capi as C
    from oracle import oracle as O
    C.load()
    O.build()
    print(json.dumps({"issued_flops": _issued_flops(C, O)}, indent=1))
