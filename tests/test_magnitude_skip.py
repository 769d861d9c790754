"""K2 leaves out the k-steps whose products lie below half the smallest denormal (extents.hip, "Magnitudes").

A product P[s][k] L[k][f] of two non-zero factors below 2^-1075 moves no accumulator: one that is 0 stays 0, one that is not
is at least 2^-1074, and all operands are non-negative.  The library bounds the matrix entries (one pass over the pools) and
the panels (propagated up the tree with the zero extents) and cuts every (16-row block, column tile) K range to the k-steps
where matrix bound + panel bound >= -1100 in log2.  Three things are pinned here:

  * every result has the bits of CAFE_NO_MAGSKIP=1 (exact-zero extents only) and of CAFE_NO_KSKIP=1 (every K tile), while
    fewer flops are issued than under CAFE_NO_MAGSKIP=1 -- a test that never skips proves nothing.  The count is
    issued_flops(): executed_flops() keeps counting the products without an exact zero in them, the rule that
    tests/test_k2_depth12.py pins from cafe_get_extents, and must not move;
  * the panel bounds dominate log2 of every entry of panels computed on the CPU, and are >= -1060 wherever an entry is not 0;
  * every K range lies inside the range the exact extents give.
"""
import numpy as np
import pytest

from cafexp_amd import problem as P, synth

pytestmark = pytest.mark.gpu

SWITCHES = ("CAFE_NO_MAGSKIP", "CAFE_NO_KSKIP", "CAFE_NO_GROUPS")


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _problem(max_count, n_families=260, n_deviations=0, n_taxa=7, seed=5):
    pb, _ = synth.make_problem(n_taxa=n_taxa, n_families=n_families, max_count=max_count, lam_sim=0.003, seed=seed,
                               root_cap=max_count // 2, n_deviations=n_deviations)
    return pb


def _context(capi, monkeypatch, pb, env=(), mus=None):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name in env:
        monkeypatch.setenv(name, "1")
    ctx = capi.Context(pb, max_categories=2)
    for name in env:
        monkeypatch.delenv(name, raising=False)
    if mus is not None:
        ctx.set_death_rates(mus)
    return ctx


def _params(oracle, pb, lam, gamma, em=None):
    prior = P.prior_uniform(pb.max_root_family_size)
    lambdas = np.full(pb.n_lambdas, lam)
    if not gamma:
        return P.Params(lambdas=lambdas, prior=prior, error_model=em)
    probs, mult = oracle.discrete_gamma(2, 0.9)
    return P.Params(lambdas=lambdas, prior=prior, multipliers=mult, cat_probs=probs, error_model=em)


def _same(a, b):
    (v1, r1), (v2, r2) = a, b
    # (the bytes, not the values: -0.0 against 0.0 or two different NaNs would be a difference)
    assert np.float64(v1).tobytes() == np.float64(v2).tobytes()
    assert r1.keys() == r2.keys()
    for key in r1:
        assert np.asarray(r1[key]).tobytes() == np.asarray(r2[key]).tobytes(), key


# (matrix order, environment of all three contexts, death rates, error model)
CASES = {
    "order751": (600, (), False, False),
    "order257": (205, (), False, False),
    "order751_no_groups": (600, ("CAFE_NO_GROUPS",), False, False),
    "order257_no_groups": (205, ("CAFE_NO_GROUPS",), False, False),
    "order751_lambda_mu": (600, (), True, False),
    "order751_error_model": (600, (), False, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_results_have_the_bits_of_the_exact_extents_and_fewer_flops_run(capi, oracle, monkeypatch, case):
    """-lnL and every family_results array of a gamma call (K = 2) and a base call, byte for byte, between the default
    context, CAFE_NO_MAGSKIP=1 and CAFE_NO_KSKIP=1; the default issues strictly fewer flops than CAFE_NO_MAGSKIP=1, except
    with an error model, where the call falls back to the exact extents and issues the same.  executed_flops(), the count of
    the products without an exact zero, is the same in both and is what CAFE_NO_MAGSKIP=1 issues."""
    max_count, env, lm, err = CASES[case]
    pb = _problem(max_count, n_deviations=3 if err else 0)
    assert pb.matrix_size == 751 if max_count == 600 else 256 <= pb.matrix_size < 272
    em = P.error_model_table(P.default_error_model(pb.max_family_size)[:1] + [[0.05, 0.9, 0.05]], pb.max_family_size) if err else None
    mus = np.full(pb.n_lambdas, 0.0012) if lm else None
    calls = [(_params(oracle, pb, 0.002, True, em), 0.9), (_params(oracle, pb, 0.0015, False, em), 1.0)]
    ctxs = {name: _context(capi, monkeypatch, pb, env + extra, mus)
            for name, extra in (("default", ()), ("no_magskip", ("CAFE_NO_MAGSKIP",)), ("no_kskip", ("CAFE_NO_KSKIP",)))}
    for pr, alpha in calls:
        got, flops, exact = {}, {}, {}
        for name, ctx in ctxs.items():
            got[name] = ctx.score(pr, alpha=alpha, per_family=True)
            flops[name] = ctx.issued_flops()
            exact[name] = ctx.executed_flops()
            if name != "no_kskip":
                assert ctx.plan_check()[0] == ctx.stats()["gemm_launches"] > 0
        print(case, "K =", 1 if pr.multipliers is None else len(pr.multipliers), "issued flops:", flops, "without an exact zero:", exact)
        assert np.isfinite(got["default"][0])
        _same(got["default"], got["no_magskip"])
        _same(got["default"], got["no_kskip"])
        assert flops["no_magskip"] < flops["no_kskip"]
        assert exact["default"] == exact["no_magskip"] == flops["no_magskip"] and exact["no_kskip"] == flops["no_kskip"]
        if err:
            assert flops["default"] == flops["no_magskip"]
        else:
            assert flops["default"] < flops["no_magskip"]


def _interior_non_root(pb):
    return [v for v in range(len(pb.parent)) if pb.leaf_taxon[v] < 0 and pb.parent[v] >= 0]


def test_panel_bounds_dominate_panels_computed_on_the_cpu(capi, oracle, monkeypatch):
    """The panels of 8 families, built on the CPU from oracle.build_matrix(..., fast=True) and numpy products.  The table has
    fewer than 128 families, so every node's panel is ONE column tile and the family's tile is tile 0.  The bound of rows
    4 r .. 4 r + 3 is >= log2 of every computed entry there, and >= -1060 wherever an entry is not zero."""
    pb = _problem(600, n_families=100)
    assert pb.matrix_size == 751 and pb.counts.shape[0] <= 128
    pr = _params(oracle, pb, 0.002, True)
    ctx = _context(capi, monkeypatch, pb)
    ctx.score(pr, alpha=0.9)
    n, M = pb.matrix_size, pb.max_family_size
    fams = np.unique(np.linspace(0, pb.counts.shape[0] - 1, 8).astype(np.int64))
    children = [[] for _ in pb.parent]
    for v, p in enumerate(pb.parent):
        if p >= 0:
            children[p].append(v)
    checked = underflowing = 0
    for k, mult in enumerate(pr.multipliers):
        mats = {v: oracle.build_matrix(n, float(pr.lambdas[pb.lambda_index[v]] * mult), float(pb.branch_length[v]), fast=True)
                for v in range(len(pb.parent)) if pb.parent[v] >= 0}
        panels = {}
        for v in range(len(pb.parent)):                      # children come before their parents
            if pb.leaf_taxon[v] >= 0 or pb.parent[v] < 0:
                continue
            L = np.ones((M + 1, len(fams)))
            for u in children[v]:
                if pb.leaf_taxon[u] >= 0:
                    L *= mats[u][:M + 1, pb.counts[fams, pb.leaf_taxon[u]]]
                else:
                    L *= mats[u][:M + 1, :M + 1] @ panels[u]
            panels[v] = L
            bound = ctx.panel_bounds(v, k)
            assert bound.shape[0] == 1 and bound.shape[1] * 4 >= M + 1
            top = L.max(axis=1)                              # per row, over the families
            for r in range((M + 1 + 3) // 4):
                m = top[4 * r:4 * r + 4].max()
                if m > 0:
                    assert bound[0, r] >= np.log2(m), (v, k, r)
                    assert bound[0, r] >= -1060, (v, k, r)
                    checked += 1
                    underflowing += m < 1e-290
    assert checked > 1000 and underflowing > 0               # (the bounds were tried on entries near the edge of fp64)


@pytest.mark.parametrize("max_count", [600, 205])
def test_every_range_lies_inside_the_range_of_the_exact_extents(capi, oracle, monkeypatch, max_count):
    """The K ranges read back after the same call from a default context and from CAFE_NO_MAGSKIP=1: per (node, category,
    column tile, 16-row block) the new range is empty or inside the old one, and some are strictly shorter."""
    pb = _problem(max_count)
    pr = _params(oracle, pb, 0.002, True)
    new_ctx, old_ctx = _context(capi, monkeypatch, pb), _context(capi, monkeypatch, pb, ("CAFE_NO_MAGSKIP",))
    new_ctx.score(pr, alpha=0.9)
    old_ctx.score(pr, alpha=0.9)
    shorter = 0
    for v in _interior_non_root(pb):
        for k in range(2):
            new, old = new_ctx.k_ranges(v, k).astype(np.int64), old_ctx.k_ranges(v, k).astype(np.int64)
            assert new.shape == old.shape and new.shape[0] >= 1
            some = new[..., 1] >= new[..., 0]
            was = old[..., 1] >= old[..., 0]
            assert not (some & ~was).any()
            assert (new[..., 0][some] >= old[..., 0][some]).all() and (new[..., 1][some] <= old[..., 1][some]).all()
            shorter += int((np.where(some, new[..., 1] - new[..., 0] + 1, 0) < np.where(was, old[..., 1] - old[..., 0] + 1, 0)).sum())
    assert shorter > 0
