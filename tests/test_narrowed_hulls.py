"""Narrowed hulls (extents_level.h, node_level_kernel; ExtNode::narrow).

Beside the structural hull of a 128-column tile -- the rows outside which a panel is exactly zero by the supports of the
matrices -- the level kernel keeps a second interval: the hull cut back from both ends over the steps of 4 rows whose
magnitude bound, BEFORE the floor of -1050, lies below 2^-1100.  Such rows hold computed zeros only.  The level above sums a
child's k-steps over the child's narrowed interval, range_kernel takes it for the panel's extent, and the assemble passes
write no row outside it.  CAFE_NO_NARROW=1 keeps the structural hulls.  Pinned here:

  * every result has the bits of CAFE_NO_NARROW=1, CAFE_NO_MAGSKIP=1 and CAFE_NO_KSKIP=1, over rate models, root rules,
    missing cells, grouped and single launches, K-tile depths and tile heights -- in cases that are asserted to narrow;
  * rows an earlier call wrote and a later call leaves outside its narrowed hulls do not leak into the call after that;
  * the rule itself, against panels computed on the CPU from the device's own matrices: every entry inside the structural
    hull and outside the narrowed one is exactly 0.0, the bounds still dominate every entry, the K ranges lie inside those of
    CAFE_NO_NARROW=1, and the families with denormal root likelihoods keep every bit of their root panels.

The tables are those of synth.make_problem: most families small (root sizes geometric, mean 50), family 0 at the largest
count, so that the column tiles of the sorted table differ and far rows fall below 2^-1100 long before they are exactly 0.
"""
import dataclasses

import numpy as np
import pytest

from cafexp_amd import problem as P, synth
import magskip_ref as R
from test_magnitude_audit import _audit_problem, _categories, _root_panels
from test_magnitude_skip import _same

pytestmark = pytest.mark.gpu

SWITCHES = ("CAFE_NO_NARROW", "CAFE_NO_MAGSKIP", "CAFE_NO_KSKIP", "CAFE_NO_GROUPS", "CAFE_KB", "CAFE_NO_ASM_SKIP")
OTHERS = (("no_narrow", {"CAFE_NO_NARROW": "1"}), ("no_magskip", {"CAFE_NO_MAGSKIP": "1"}), ("no_kskip", {"CAFE_NO_KSKIP": "1"}))


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _problem(max_count, n_families, n_taxa, two_lambdas=False, missing=False):
    pb, _ = synth.make_problem(n_taxa=n_taxa, n_families=n_families, max_count=max_count, lam_sim=0.003, seed=5, root_cap=max_count // 2,
                               lambda_clade_min=3 if two_lambdas else 0)
    assert pb.matrix_size == (751 if max_count == 600 else 257) and pb.n_lambdas == (2 if two_lambdas else 1)
    if missing:
        # Every second family of the quarter with the smallest largest counts loses one cell, the taxon moving along.  (A
        # missing leaf's factor is 1.0 in every row: next to such a column a tile's leaf bound is that of 1.0 and cuts nothing.
        # The columns stand in the order of their largest count, so the tiles of the larger families hold no missing cell.)
        counts = pb.counts.copy()
        small = np.argsort(counts.max(axis=1), kind="stable")[:pb.n_families // 4]
        for i, f in enumerate(small[::2]):
            counts[f, i % counts.shape[1]] = P.COUNT_MISSING
        pb = dataclasses.replace(pb, counts=counts, missing_counts=True)
    return pb


def _context(capi, monkeypatch, pb, env=None, mus=None, plain=False, rule=None):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    ctx = capi.Context(pb, max_categories=2, dedup=not plain, subtree_dedup=not plain)
    for name in env or {}:
        monkeypatch.delenv(name, raising=False)
    if mus is not None:
        ctx.set_death_rates(mus)
    if rule is not None:
        ctx.set_root_rule(rule)
    return ctx


def _params(oracle, pb, lam, gamma, em=None):
    lambdas = np.full(pb.n_lambdas, lam) * (1.0 + 0.55 * np.arange(pb.n_lambdas))
    pr = P.Params(lambdas=lambdas, prior=P.prior_uniform(pb.max_root_family_size), error_model=em)
    if gamma:
        pr.cat_probs, pr.multipliers = oracle.discrete_gamma(2, 0.9)
    return pr


def _interior_non_root(pb):
    return [v for v in range(len(pb.parent)) if pb.leaf_taxon[v] < 0 and pb.parent[v] >= 0]


def _length(e):
    return np.where(e[..., 1] >= e[..., 0], e[..., 1].astype(np.int64) - e[..., 0] + 1, 0)


def _hulls(ctx, pb, K):
    """{(node, category): (structural hulls [tiles][2], narrowed hulls [tiles][2])} of the last call"""
    return {(v, k): (ctx.extents(v, k)[1], ctx.narrowed_extents(v, k)) for v in _interior_non_root(pb) for k in range(K)}


def _assert_narrowed(hulls):
    """Every narrowed hull lies inside its structural one; returns (tiles cut back, tiles cut away whole, rows cut)."""
    cut = whole = rows = 0
    for key, (s, n) in hulls.items():
        assert s.shape == n.shape and s.shape[0] > 0, key
        ls, ln = _length(s), _length(n)
        some = ln > 0
        assert (ls[some] > 0).all() and (n[some, 0] >= s[some, 0]).all() and (n[some, 1] <= s[some, 1]).all(), key
        # cut in whole steps of 4 rows, or at the structural end
        assert ((n[some, 0] % 4 == 0) | (n[some, 0] == s[some, 0])).all() and ((n[some, 1] % 4 == 3) | (n[some, 1] == s[some, 1])).all(), key
        cut += int((ln < ls).sum()); whole += int(((ln == 0) & (ls > 0)).sum()); rows += int((ls - ln).sum())
    return cut, whole, rows


def _ranges(ctx, pb, K):
    return {(v, k): ctx.k_ranges(v, k).astype(np.int64) for v in _interior_non_root(pb) for k in range(K)}


def _dead_tiles(ranges, mi):
    """{(node, category): all-zero output tiles [column tile][row tile]} at tiles of `mi` 16-row blocks, from the K ranges: a
    tile none of whose blocks has a range -- what K2 takes for an all-zero tile (blocks past the matrix's last one say none)."""
    out = {}
    for key, r in ranges.items():
        some = r[..., 1] >= r[..., 0]
        some = np.pad(some, ((0, 0), (0, (-some.shape[1]) % mi)))
        out[key] = ~some.reshape(some.shape[0], -1, mi).any(axis=2)
    return out


def _tile_heights(ctx):
    return sorted(set(int(m) for m in ctx.launch_flops()[2]))


def _assert_inside(new, old):
    """Every K range of `new` lies inside that of `old`; returns how many are strictly shorter."""
    shorter = 0
    for key in old:
        n, o = new[key], old[key]
        assert n.shape == o.shape
        some, was = n[..., 1] >= n[..., 0], o[..., 1] >= o[..., 0]
        assert not (some & ~was).any(), key
        assert (n[..., 0][some] >= o[..., 0][some]).all() and (n[..., 1][some] <= o[..., 1][some]).all(), key
        shorter += int((np.where(some, n[..., 1] - n[..., 0] + 1, 0) < np.where(was, o[..., 1] - o[..., 0] + 1, 0)).sum())
    return shorter


def _with_large_families(pb, n, seed=3):
    """pb with n families appended whose size is drawn from the upper fifth of the table's range, every count within 3 of it.
    The columns stand in the order of their largest count, so these fill column tiles of their own: a band of live rows
    around their sizes, all-zero output tiles below it (at least the rows up to half the largest count) and above it."""
    rng = np.random.default_rng(seed)
    top = int(pb.counts.max())
    size = rng.integers(top * 4 // 5, top - 20, size=(n, 1))
    big = (size + rng.integers(-3, 4, size=(n, pb.counts.shape[1]))).astype(pb.counts.dtype)
    return dataclasses.replace(pb, counts=np.ascontiguousarray(np.vstack([pb.counts, big])), family_ids=list(pb.family_ids) + ["big%d" % i for i in range(n)])


# name: (largest count, families, taxa, environment of every context, death rates, two lambdas, root rule, missing cells)
CASES = {
    "order751": (600, 700, 14, {}, False, False, None, False),
    "order257": (205, 300, 12, {}, False, False, None, False),
    "order751_1500_families": (600, 1500, 12, {}, False, False, None, False),
    "order751_lambda_mu": (600, 700, 14, {}, True, False, None, False),
    "order751_two_lambdas": (600, 700, 14, {}, False, True, None, False),
    "order751_sum_rule": (600, 700, 14, {}, False, False, "sum", False),
    "order257_sum_rule": (205, 300, 12, {}, False, False, "sum", False),
    "order751_missing": (600, 700, 14, {}, False, False, None, True),
    "order257_missing": (205, 700, 14, {}, False, False, None, True),
    "order751_no_groups": (600, 700, 14, {"CAFE_NO_GROUPS": "1"}, False, False, None, False),
    "order257_no_groups": (205, 300, 12, {"CAFE_NO_GROUPS": "1"}, False, False, None, False),
    "order751_kb8": (600, 700, 14, {"CAFE_KB": "8"}, False, False, None, False),
    "order751_kb12": (600, 700, 14, {"CAFE_KB": "12"}, False, False, None, False),
    "order751_kb16": (600, 700, 14, {"CAFE_KB": "16"}, False, False, None, False),
    "order257_kb16": (205, 300, 12, {"CAFE_KB": "16"}, False, False, None, False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_results_have_the_bits_of_the_structural_hulls(capi, oracle, monkeypatch, case):
    """A gamma call (K = 2) and a base call: -lnL, every family_results array and every root panel byte for byte between the
    default context and CAFE_NO_NARROW=1, CAFE_NO_MAGSKIP=1, CAFE_NO_KSKIP=1.  First the case is shown to be one: some tile's
    hull is cut back, the hulls of CAFE_NO_NARROW=1 are the structural ones, the default's K ranges lie inside those of
    CAFE_NO_NARROW=1 with some strictly shorter, and it issues fewer flops; the tile lists still match the ranges."""
    max_count, n_families, n_taxa, env, lm, two, rule, missing = CASES[case]
    pb = _with_large_families(_problem(max_count, n_families, n_taxa, two, missing), 150)    # (all-zero output tiles at any height)
    mus = np.full(pb.n_lambdas, 0.0012) if lm else None
    ctxs = {"default": _context(capi, monkeypatch, pb, env, mus, rule=rule)}
    for name, extra in OTHERS:
        ctxs[name] = _context(capi, monkeypatch, pb, dict(env, **extra), mus, rule=rule)
    for pr, alpha in [(_params(oracle, pb, 0.002, True), 0.9), (_params(oracle, pb, 0.0015, False), 1.0)]:
        K = _categories(pr)
        got, roots, flops = {}, {}, {}
        for name, ctx in ctxs.items():
            got[name] = ctx.score(pr, alpha=alpha, per_family=True)
            roots[name] = _root_panels(ctx, pb, pr)
            flops[name] = ctx.issued_flops()
            if name != "no_kskip":
                assert ctx.plan_check()[0] == ctx.stats()["gemm_launches"] > 0
        cut, whole, rows = _assert_narrowed(_hulls(ctxs["default"], pb, K))
        assert _assert_narrowed(_hulls(ctxs["no_narrow"], pb, K)) == (0, 0, 0)
        assert _assert_narrowed(_hulls(ctxs["no_magskip"], pb, K)) == (0, 0, 0)
        shorter = _assert_inside(_ranges(ctxs["default"], pb, K), _ranges(ctxs["no_narrow"], pb, K))
        heights = _tile_heights(ctxs["default"])
        dead = sum(int(d.sum()) for mi in heights for d in _dead_tiles(_ranges(ctxs["default"], pb, K), mi).values())
        was = sum(int(d.sum()) for mi in heights for d in _dead_tiles(_ranges(ctxs["no_narrow"], pb, K), mi).values())
        print(case, "K =", K, "tiles cut back:", cut, "cut away whole:", whole, "rows cut:", rows, "K ranges shorter:", shorter,
              "all-zero output tiles at heights", heights, ":", dead, "with structural hulls:", was, "issued flops:", flops)
        assert cut > 0 and rows > 0 and shorter > 0
        # all-zero output tiles, no fewer than the structural hulls give.  (Asserted to exist at order 751 only: a matrix of
        # order 257 spans too few binades for a whole 32-row tile to fall below 2^-1100 next to families of up to 205 -- these
        # tables have no such tile at that order under either rule; there the case must still narrow, above.)
        assert dead >= was and (dead > 0 or max_count != 600)
        assert flops["default"] < flops["no_narrow"] <= flops["no_magskip"] < flops["no_kskip"]
        assert ctxs["default"].executed_flops() == ctxs["no_narrow"].executed_flops() == flops["no_magskip"]
        assert np.isfinite(got["default"][0]) and roots["default"].any()
        for name, _ in OTHERS:
            _same(got["default"], got[name])
            assert roots["default"].tobytes() == roots[name].tobytes(), name
    for ctx in ctxs.values():
        ctx.close()


@pytest.mark.parametrize("max_count,n_families,n_taxa", [(600, 700, 14), (205, 300, 12)])
def test_every_tile_height_has_the_bits_of_the_structural_hulls(capi, oracle, monkeypatch, max_count, n_families, n_taxa):
    """force_tile(2 .. 9), every height it accepts, on one default context and one of CAFE_NO_NARROW=1: the gamma call's
    results and root panels byte for byte, at every height those of the first; the narrowing does not depend on the height."""
    pb = _problem(max_count, n_families, n_taxa)
    pr = _params(oracle, pb, 0.002, True)
    new, old = _context(capi, monkeypatch, pb), _context(capi, monkeypatch, pb, {"CAFE_NO_NARROW": "1"})
    first = hulls = None
    for mi in range(2, 10):
        new.force_tile(mi); old.force_tile(mi)
        a, b = new.score(pr, alpha=0.9, per_family=True), old.score(pr, alpha=0.9, per_family=True)
        assert new.plan_check()[0] == new.stats()["gemm_launches"] > 0
        _same(a, b)
        ra, rb = _root_panels(new, pb, pr), _root_panels(old, pb, pr)
        assert ra.tobytes() == rb.tobytes(), mi
        h = _hulls(new, pb, 2)
        assert _assert_narrowed(h)[0] > 0 and new.issued_flops() < old.issued_flops()
        if first is None:
            first, hulls = (a, ra), h
        _same(a, first[0])
        assert ra.tobytes() == first[1].tobytes()
        assert all(h[key][1].tobytes() == hulls[key][1].tobytes() for key in h)
    new.close(); old.close()


def test_a_call_with_an_error_model_between_two_without_keeps_the_structural_hulls(capi, oracle, monkeypatch):
    """A context created with an error model: every scorer call of it carries the model and keeps no magnitude tables, its
    call without one is root_max.  root_max, a gamma call with the 3-tap model, root_max again on one context: the model's
    call narrows nothing -- its narrowed hulls read back as the structural ones -- the two others do, and each has the bits
    of a fresh CAFE_NO_NARROW=1 context given that call alone."""
    pb, _ = synth.make_problem(n_taxa=14, n_families=700, max_count=600, lam_sim=0.003, seed=5, root_cap=300, n_deviations=3)
    em = P.error_model_table(P.default_error_model(pb.max_family_size)[:1] + [[0.05, 0.9, 0.05]], pb.max_family_size)
    gamma, base = _params(oracle, pb, 0.002, True, em), _params(oracle, pb, 0.002, False, em)
    plain = lambda c: (np.asarray(c.root_max(np.array([0.002]))), {})
    steps = [(plain, base), (lambda c: c.score(gamma, alpha=0.9, per_family=True), gamma), (plain, base)]
    ctx = _context(capi, monkeypatch, pb)
    cuts = []
    for run, pr in steps:
        got, roots = run(ctx), _root_panels(ctx, pb, pr)
        cuts.append(_assert_narrowed(_hulls(ctx, pb, _categories(pr)))[0])
        fresh = _context(capi, monkeypatch, pb, {"CAFE_NO_NARROW": "1"})
        want = run(fresh)
        assert np.asarray(got[0]).tobytes() == np.asarray(want[0]).tobytes() and got[1].keys() == want[1].keys()
        assert all(np.asarray(got[1][key]).tobytes() == np.asarray(want[1][key]).tobytes() for key in got[1])
        assert roots.any() and roots.tobytes() == _root_panels(fresh, pb, pr).tobytes()
        fresh.close()
    ctx.close()
    print("tiles cut back per call:", cuts)
    assert cuts[0] > 0 and cuts[1] == 0 and cuts[2] == cuts[0]


@pytest.mark.parametrize("max_count,n_families,n_taxa", [(600, 700, 14), (205, 300, 12)])
def test_rows_outside_a_narrowed_hull_do_not_leak_into_the_next_call(capi, oracle, monkeypatch, max_count, n_families, n_taxa):
    """One context scored with wide (lambda 0.01), narrow (0.0005), wide parameters, base model: each call has the bits of a
    fresh context's.  The assemble passes of the narrow call leave the rows outside its narrowed hulls as the wide call wrote
    them; asserted first: at some tile the wide call's narrowed hull reaches beyond the narrow call's, at a node whose panel an
    assemble pass writes or not -- every node counts, the K ranges must keep out of those rows either way."""
    pb = _problem(max_count, n_families, n_taxa)
    ctx = _context(capi, monkeypatch, pb)
    seen, results = [], []
    for lam in (0.01, 0.0005, 0.01):
        pr = _params(oracle, pb, lam, False)
        results.append((ctx.score(pr, alpha=1.0, per_family=True), _root_panels(ctx, pb, pr)))
        seen.append(_hulls(ctx, pb, 1))
        fresh = _context(capi, monkeypatch, pb)
        _same(results[-1][0], fresh.score(pr, alpha=1.0, per_family=True))
        assert results[-1][1].tobytes() == _root_panels(fresh, pb, pr).tobytes(), lam
        fresh.close()
    ctx.close()
    assert _assert_narrowed(seen[1])[0] > 0
    beyond = 0
    for key in seen[0]:
        w, n = seen[0][key][1].astype(np.int64), seen[1][key][1].astype(np.int64)
        both = (_length(w) > 0)
        lo = np.where(_length(n) > 0, n[:, 0], 1 << 30); hi = np.where(_length(n) > 0, n[:, 1], -1)
        beyond += int((both & ((w[:, 0] < lo) | (w[:, 1] > hi))).sum())
    print("tiles whose rows of the wide call lie outside the narrow call's narrowed hull:", beyond)
    assert beyond > 0
    _same(results[0][0], results[2][0])
    assert results[0][1].tobytes() == results[2][1].tobytes()


@pytest.mark.parametrize("name", ["order751", "order257_12_taxa", "order751_lambda_mu", "order751_two_lambdas"])
def test_every_row_the_narrowing_cuts_is_zero_in_panels_computed_on_the_cpu(capi, oracle, monkeypatch, name):
    """The problems of tests/test_magnitude_audit.py (families in the order of their largest count, the families with denormal
    root likelihoods in the third column tile), contexts without dedup and subtree dedup so that panel column f is family f.
    With L_v the panel of node v computed on the CPU from the DEVICE's matrices of the call: every entry of every row inside
    the structural hull of a tile and outside its narrowed hull is exactly 0.0 (some such rows exist), panel_bounds dominates
    every entry, the K ranges lie inside those of CAFE_NO_NARROW=1, and scores and root panels -- the denormal ones among
    them -- have the bits of CAFE_NO_NARROW=1."""
    pb, edge, pr = _audit_problem(oracle, name)
    from test_magnitude_audit import AUDIT
    mus = AUDIT[name][3]
    F, M, K = pb.n_families, pb.max_family_size, _categories(pr)
    n_tiles = (F + 127) // 128
    alpha = 0.9 if K > 1 else 1.0
    new = _context(capi, monkeypatch, pb, mus=mus, plain=True)
    old = _context(capi, monkeypatch, pb, {"CAFE_NO_NARROW": "1"}, mus=mus, plain=True)
    v_new, v_old = new.score(pr, alpha=alpha, per_family=True), old.score(pr, alpha=alpha, per_family=True)
    hulls = _hulls(new, pb, K)
    cut, whole, rows_cut = _assert_narrowed(hulls)
    assert _assert_narrowed(_hulls(old, pb, K)) == (0, 0, 0)
    checked = 0
    for k in range(K):
        mats = {v: new.matrix(v, k) for v in range(pb.n_nodes) if pb.parent[v] >= 0}
        panels = R.cpu_panels(pb, mats, pb.counts)
        for v in R.interior_non_root(pb):
            L = panels[v]
            s, n = hulls[v, k]
            assert L.shape == (M + 1, F) and s.shape[0] == n_tiles
            Lp = np.zeros((M + 1, 128 * n_tiles))
            Lp[:, :F] = L
            for ct in range(n_tiles):
                T = Lp[:, 128 * ct:128 * ct + 128]
                inside = np.zeros(M + 1, dtype=bool)
                if s[ct, 1] >= s[ct, 0]:
                    inside[s[ct, 0]:s[ct, 1] + 1] = True
                assert not T[~inside].any(), (v, k, ct)       # (the structural hull itself)
                if n[ct, 1] >= n[ct, 0]:
                    inside[n[ct, 0]:n[ct, 1] + 1] = False
                assert not T[inside].any(), (v, k, ct, float(T[inside].max()))
                checked += int(inside.sum())
            bound = new.panel_bounds(v, k)
            Lq = np.zeros((4 * bound.shape[1], 128 * n_tiles))
            Lq[:M + 1] = Lp
            top = R._log2(Lq.reshape(bound.shape[1], 4, n_tiles, 128).max(axis=(1, 3))).T
            assert (bound >= top).all(), (v, k)
    shorter = _assert_inside(_ranges(new, pb, K), _ranges(old, pb, K))
    print(name, "tiles cut back:", cut, "cut away whole:", whole, "rows cut:", rows_cut, "rows checked to be zero:", checked, "K ranges shorter:", shorter)
    assert cut > 0 and checked == rows_cut > 0 and shorter > 0
    _same(v_new, v_old)
    r_new, r_old = _root_panels(new, pb, pr), _root_panels(old, pb, pr)
    assert r_new.tobytes() == r_old.tobytes()
    if len(edge):
        assert ((r_new[edge] > 0) & (r_new[edge] < R.TINY)).any()    # denormal entries were compared
    new.close(); old.close()


@pytest.mark.parametrize("max_count,n_families,n_taxa,gamma", [(600, 700, 14, True), (600, 700, 14, False), (600, 260, 12, False)])
def test_all_zero_tiles_at_every_place_of_an_ops_tile_order_receive_their_zeros(capi, oracle, monkeypatch, max_count, n_families, n_taxa, gamma):
    """More than half of the bench call's output tiles are all-zero once the hulls are narrowed: no block of the tile has a K
    range, K2 fetches the one K tile of its list entry, multiplies nothing and stores the epilogue's zeros (and, at row tile 0
    of an interior parent's op, row 0 of the panel).  A table with 300 large families in column tiles of their own, at every
    tile height force_tile accepts: -lnL, every family_results array and every root panel byte for byte against
    CAFE_NO_NARROW=1 and CAFE_NO_KSKIP=1, and the lists pass plan_check.  A workgroup's list holds an op's tiles row tile
    fastest, so what is asserted from the K ranges, per height, places the tiles: an all-zero tile at row tile 0 (first of its
    column's tiles, with the row-0 write), one at the last row tile, two or more in a row followed by a live one, a live one
    followed by an all-zero one.  Where a tile stands in a workgroup's list, and which epilogue variant its op runs (store,
    multiply, fused leaf, gathered factor, transposed: a Yule tree of 12 to 14 taxa has nodes of every kind), is not read back:
    the variants run together and are not told apart here."""
    pb = _with_large_families(_problem(max_count, n_families, n_taxa), 300)
    pr = _params(oracle, pb, 0.002, gamma)
    K, alpha = _categories(pr), 0.9 if gamma else 1.0
    new = _context(capi, monkeypatch, pb)
    old = _context(capi, monkeypatch, pb, {"CAFE_NO_NARROW": "1"})
    full = _context(capi, monkeypatch, pb, {"CAFE_NO_KSKIP": "1"})
    want = full.score(pr, alpha=alpha, per_family=True)
    want_roots = _root_panels(full, pb, pr)
    full.close()
    for mi in range(2, 10):
        new.force_tile(mi); old.force_tile(mi)
        a, b = new.score(pr, alpha=alpha, per_family=True), old.score(pr, alpha=alpha, per_family=True)
        assert new.plan_check()[0] == new.stats()["gemm_launches"] > 0 and old.plan_check()[0] > 0
        dead = _dead_tiles(_ranges(new, pb, K), mi)
        n_rt = -(-pb.max_family_size // (16 * mi))           # row tiles of an interior parent's op: parent sizes 1 .. M
        seen = dict(first=0, last=0, run_then_live=0, live_then_dead=0, tiles=0)
        for d in dead.values():
            d = d[:, :n_rt]
            seen["tiles"] += int(d.sum())
            seen["first"] += int(d[:, 0].sum()); seen["last"] += int(d[:, -1].sum())
            if n_rt >= 3:
                seen["run_then_live"] += int((d[:, :-2] & d[:, 1:-1] & ~d[:, 2:]).sum())
            seen["live_then_dead"] += int((~d[:, :-1] & d[:, 1:]).sum())
        print("height", mi, "row tiles", n_rt, seen)
        # (the large families' sizes are at least 4/5 of the largest count, 480; the lower tail of their band, through up to
        # five levels of branches, is taken to end above a quarter of it: rows 1 .. 150 are all-zero in their column tiles,
        # which holds one tile of every height, and two of the heights up to 64 rows)
        top = int(pb.counts.max())
        assert top == 600 and seen["tiles"] > 0 and seen["last"] > 0 and seen["live_then_dead"] > 0 and seen["first"] > 0
        assert seen["run_then_live"] > 0 or 32 * mi > top // 4
        _same(a, b); _same(a, want)
        ra, rb = _root_panels(new, pb, pr), _root_panels(old, pb, pr)
        assert ra.any() and ra.tobytes() == rb.tobytes() == want_roots.tobytes(), mi
    new.close(); old.close()
