"""Audit of the k-steps that K2's magnitude rule leaves out (extents.hip, "Magnitudes"), at the edge of fp64.

tests/test_magnitude_skip.py compares scores of ordinary families, whose likelihoods lie 200 decades above the products the
rule drops: a bound wrong by hundreds of bits, a swapped tile index or a stale table would pass there.  Three things here:

  1. families whose largest root likelihood is DENORMAL or just above (copies of the table's largest family with one tip
     lowered, chosen with the CPU oracle): scores and the root panels themselves, denormal entries included, have the bits of
     CAFE_NO_MAGSKIP=1 and CAFE_NO_KSKIP=1; the root panels also at the shapes of tests/test_magnitude_skip.py;
  2. the proof obligation itself: for every (column tile, 16-row block, k-step) inside the range of the exact extents and
     outside the issued range, (largest matrix entry of the block in the step) x (largest panel entry of the step in the tile)
     < 2^-1077, from the DEVICE's matrices of the call and panels computed from them on the CPU, over three column tiles,
     several trees, rate models and orders up to 2048; and the panel bounds against every entry of those panels;
  3. the tables are those of the call, not of the previous one: sequences of calls on one context against fresh contexts.

What depends on the reference alone -- the bands of the edge families, column = family, that skipped steps hold non-zero
products -- is asserted before anything is compared with the device.
"""
import dataclasses
import json
import os

import numpy as np
import pytest

from cafexp_amd import problem as P, synth
from helpers import _explicit_problem
import magskip_ref as R
from test_magnitude_skip import CASES, SWITCHES, _context, _params, _problem, _same

gpu = pytest.mark.gpu

VEC_TOL = 5e-11                  # the suite's tolerance of a likelihood against the oracle (tests/test_large_orders.py)
N_ORDINARY = 248                 # families of a table before its 8 + up to 8 edge families: the last ones fill the third column tile alone


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _ctx(capi, monkeypatch, pb, env=(), mus=None, plain=False):
    """_context of tests/test_magnitude_skip.py; plain: without dedup and subtree dedup, one panel column per family."""
    if not plain:
        return _context(capi, monkeypatch, pb, env, mus)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name in env:
        monkeypatch.setenv(name, "1")
    ctx = capi.Context(pb, max_categories=2, dedup=False, subtree_dedup=False)
    for name in env:
        monkeypatch.delenv(name, raising=False)
    if mus is not None:
        ctx.set_death_rates(mus)
    return ctx


def _three(capi, monkeypatch, pb, env=(), mus=None, plain=False):
    return {name: _ctx(capi, monkeypatch, pb, env + extra, mus, plain)
            for name, extra in (("default", ()), ("no_magskip", ("CAFE_NO_MAGSKIP",)), ("no_kskip", ("CAFE_NO_KSKIP",)))}


def _categories(pr):
    return 1 if pr.multipliers is None else len(pr.multipliers)


def _root_panels(ctx, pb, pr):
    """[family][category][R]: the root panel as the last call left it."""
    return np.array([[ctx.root_likelihoods(f, k) for k in range(_categories(pr))] for f in range(pb.n_families)])


def _sample(pb, idx):
    return dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[idx]), family_ids=[pb.family_ids[i] for i in idx])


# ------------------------------------------------------------------ the CPU side, tested on its own (no device)
def test_the_audit_sees_a_planted_violation_and_passes_what_underflows():
    """audit_skipped_steps on a hand-made op: a skipped step whose product is 2^-1200 passes, one at 2^-1000 is reported, and
    steps outside the exact range or inside the issued range do not count."""
    M, n = 31, 40
    P_ = np.zeros((n, n))
    L = np.zeros((M + 1, 130))                               # two column tiles
    P_[17:33, 0:4] = 2.0 ** -600                             # block 1 (sizes 17 .. 32), k-step 0
    P_[17:33, 4:8] = 2.0 ** -500                             # block 1, k-step 1
    P_[20, 8:12] = 1.0                                       # block 1, k-step 2
    L[0:4, 129] = 2.0 ** -600                                # tile 1, k-step 0: product 2^-1200
    L[5, 128] = 2.0 ** -500                                  # tile 1, k-step 1: product 2^-1000
    L[8:12, :] = 0.5
    nb = (n - 1 + 15) // 16
    old = np.zeros((2, nb, 2), dtype=np.int32)
    old[..., 0], old[..., 1] = 1, 0                          # (none)
    old[1, 1] = (0, 2)
    new = old.copy()
    new[1, 1] = (1, 2)                                       # k-step 0 left out
    assert R.audit_skipped_steps(P_, L, M, new, old) == (1, 1, -1200.0, (1, 1, 0))
    new[1, 1] = (2, 2)                                       # k-steps 0 and 1 left out
    n_skipped, n_nonzero, worst, where = R.audit_skipped_steps(P_, L, M, new, old)
    assert (n_skipped, n_nonzero, worst, where) == (2, 2, -1000.0, (1, 1, 1)) and not worst < R.SKIP_LOG2
    new[0, 1] = (0, 0)                                       # a range that is not inside the exact one
    with pytest.raises(AssertionError):
        R.audit_skipped_steps(P_, L, M, new, old)
    # log2 of denormals, which the comparison relies on
    assert R._log2(np.array([5e-324, 0.0]))[0] == -1074.0 and R._log2(np.array([5e-324, 0.0]))[1] == -np.inf


def test_the_panels_of_the_helper_are_the_oracles(oracle):
    """cpu_panels from the oracle's matrices against oracle.prune, and the band conditions of edge_rows by the oracle alone
    (a small table: the bands themselves are asserted at the tests' own shapes, on the GPU machine, before any comparison)."""
    pb = _problem(60, n_families=20)
    lambdas = np.array([0.004])
    pr = P.Params(lambdas=lambdas, prior=P.prior_uniform(pb.max_root_family_size))
    root = R.cpu_panels(pb, R.oracle_matrices(oracle, pb, lambdas), pb.counts)[R.root_of(pb)]
    assert root.shape == (pb.max_root_family_size, pb.n_families)
    for f in range(pb.n_families):
        want = oracle.prune(pb, pr, f, fast=True)
        assert np.abs(root[:, f] - want).max() <= 1e-12 * want.max()
    pb2, idx = R.with_rows(pb, np.array([pb.counts[0]]), sort=True)
    assert (np.diff(pb2.counts.max(axis=1)) >= 0).all() and (pb2.counts[idx[0]] == pb.counts[0]).all()


# ------------------------------------------------------------------ 1. families at the edge of fp64
_edge_cache = {}


def _edge_case(oracle, call):
    """_problem(600) with the edge families of `call` appended (copies of family 0 with one tip lowered), the call's
    parameters and what the oracle says of them: with its fast matrices, computed here, and with its exact ones, recorded in
    tests/golden/ref_magnitude_audit.json (half a minute per call).  The bands are asserted on the oracle alone
    (edge_problem).  Built once per call and shared.

    The table has N_ORDINARY = 248 families of its own and 8 edge families of either band, so that in a context without dedup
    the denormal ones fill the third column tile ALONE (edge_problem says why that matters)."""
    if call in _edge_cache:
        return _edge_cache[call]
    lam, gamma = R.CALLS[call]
    pb0 = _problem(600, n_families=N_ORDINARY)
    assert pb0.matrix_size == 751 and pb0.n_families == N_ORDINARY
    pr = _params(oracle, pb0, lam, gamma)
    assert not gamma or pr.multipliers.tolist() == oracle.discrete_gamma(2, R.ALPHA)[1].tolist()
    pb, idx, tops, n_first = R.edge_problem(oracle, pb0, pr)
    print(call, "edge families: largest root likelihood per category", tops.tolist())
    assert 12 <= len(idx) <= 20 and pb.matrix_size == 751
    assert ((pb.counts[idx] != pb0.counts[0]).sum(axis=1) == 1).all()          # one tip lowered
    assert N_ORDINARY + n_first == 256 and (np.argsort(pb.counts.max(axis=1), kind="stable")[N_ORDINARY:] == idx).all()
    sub = _sample(pb, idx)
    with open(os.path.join(os.path.dirname(__file__), "golden", "ref_magnitude_audit.json")) as f:
        exact = json.load(f)["calls"][call]
    assert exact["rows"] == sub.counts.tolist() and exact["lambda"] == lam, "the fixture is not of these families: run its generator"
    if gamma:
        _, cat, fam = oracle.score_gamma(sub, pr, fast=True, per_family=True)
        fast = {"category_likelihood": cat, "family_likelihood": fam}
    else:
        fast = {"family_lnl": oracle.score_base(sub, pr, fast=True, per_family=True)[1]}
    want = {True: fast, False: {key: np.array(exact[key]) for key in fast}}
    _edge_cache[call] = (pb, idx, pr, R.ALPHA if gamma else 1.0, want)
    return _edge_cache[call]


def _check_edge_values(call, got, want, scale):
    """got: the device's per-family arrays of the edge families; want[fast]: the oracle's with its fast and its exact
    matrices.  The tolerance of a value is the oracle's own fast-against-exact difference, the largest over the values of its
    group (printed), plus VEC_TOL, the suite's tolerance of a likelihood against the oracle.  A value below 1e-290 also gets
    (4096 scale + 2) x 2^-1074, scale = the largest prior: in the denormal range sums are exact and each product rounds by at
    most half a step, 721 products per dot product, 5 levels, device and oracle: under 4096 steps at the root vector, which
    the prior scales down, and a step for that product and the category's.  family_lnl is compared as exp(lnL)."""
    for key in want[True]:
        g, w, x = (np.asarray(a[key], dtype=np.float64) for a in (got, want[True], want[False]))
        assert g.shape == w.shape == x.shape
        if key == "family_lnl":
            g, w, x = np.exp(g), np.exp(w), np.exp(x)
        assert np.isfinite(g).all() and (g > 0).all() and (w > 0).all() and (x > 0).all(), key
        low = w < 1e-290
        for name, grp in (("above 1e-290", ~low), ("below 1e-290", low)):
            if not grp.any():
                continue
            measured = float((np.abs(w - x)[grp] / x[grp]).max())
            tol = measured + VEC_TOL + ((4096 * scale + 2) * 2.0 ** -1074 / w[grp] if name.startswith("below") else 0.0)
            err = np.abs(g - w)[grp] / w[grp]
            print(call, key, name, "(%d values) oracle fast against exact: %.3g, device against oracle: %.3g" % (grp.sum(), measured, float(err.max())))
            assert (err <= tol).all(), (key, name, err.max())


@gpu
@pytest.mark.parametrize("plain", [False, True], ids=["dedup", "no_dedup"])
@pytest.mark.parametrize("call", sorted(R.CALLS))
def test_edge_families_keep_every_bit_of_scores_and_root_panels(capi, oracle, monkeypatch, call, plain):
    """248 ordinary families and the call's edge families, in default contexts and in contexts without dedup and subtree
    dedup: -lnL, every family_results array and EVERY root panel (root_likelihoods(f, k): the panel itself, whose denormal
    entries the log-likelihood washes out) byte for byte between the default, CAFE_NO_MAGSKIP=1 and CAFE_NO_KSKIP=1, while the
    default issues strictly fewer flops; the edge families' values are finite and the oracle's."""
    pb, idx, pr, alpha, want = _edge_case(oracle, call)
    got, roots, flops = {}, {}, {}
    for name, ctx in _three(capi, monkeypatch, pb, plain=plain).items():
        got[name] = ctx.score(pr, alpha=alpha, per_family=True)
        flops[name] = ctx.issued_flops()
        roots[name] = _root_panels(ctx, pb, pr)
        ctx.close()
    print(call, "issued flops:", flops)
    for other in ("no_magskip", "no_kskip"):
        differ = np.argwhere((roots["default"].view(np.uint64) != roots[other].view(np.uint64)).any(axis=2))
        assert len(differ) == 0, (other, "root panels differ at (family, category)", differ[:8].tolist())
        _same(got["default"], got[other])
    assert np.isfinite(got["default"][0])
    assert flops["default"] < flops["no_magskip"] < flops["no_kskip"]
    # the root panels of the edge families are at the edge: denormal entries were compared
    top = roots["default"][idx].max(axis=2)
    assert R.band_counts(top)[0] >= 3 and ((roots["default"][idx] > 0) & (roots["default"][idx] < R.TINY)).sum() > 100
    _check_edge_values(call, {k: np.asarray(v)[idx] for k, v in got["default"][1].items()}, want, float(pr.prior.max()))


@gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_root_panels_have_the_bits_of_the_exact_extents(capi, oracle, monkeypatch, case):
    """The shapes and calls of test_results_have_the_bits_of_the_exact_extents_and_fewer_flops_run: every root panel, every
    family and category, byte for byte between the default, CAFE_NO_MAGSKIP=1 and CAFE_NO_KSKIP=1."""
    max_count, env, lm, err = CASES[case]
    pb = _problem(max_count, n_deviations=3 if err else 0)
    em = P.error_model_table(P.default_error_model(pb.max_family_size)[:1] + [[0.05, 0.9, 0.05]], pb.max_family_size) if err else None
    mus = np.full(pb.n_lambdas, 0.0012) if lm else None
    ctxs = _three(capi, monkeypatch, pb, env, mus)
    for pr, alpha in [(_params(oracle, pb, 0.002, True, em), 0.9), (_params(oracle, pb, 0.0015, False, em), 1.0)]:
        roots = {}
        for name, ctx in ctxs.items():
            ctx.score(pr, alpha=alpha)
            roots[name] = _root_panels(ctx, pb, pr)
        assert roots["default"].any()
        assert roots["default"].tobytes() == roots["no_magskip"].tobytes() == roots["no_kskip"].tobytes()


# ------------------------------------------------------------------ 2. every skipped k-step against the operands
# name: (largest count, taxa, lambdas, death rates, lambda_clade_min, gamma, whether the call must skip)
AUDIT = {
    "order751": (600, 7, [0.002], None, 0, True, True),
    "order257": (205, 7, [0.002], None, 0, True, True),
    "order751_lambda_mu": (600, 7, [0.002], [0.0012], 0, True, True),
    "order751_two_lambdas": (600, 7, [0.002, 0.0031], None, 3, True, True),
    "order257_12_taxa": (205, 12, [0.002], None, 0, True, True),
    "order751_narrow_bands": (600, 7, [0.0005], None, 0, False, True),
    # (at lambda = 0.01 the bands are broad; whether anything is left to skip is not this test's business, the audit is)
    "order257_broad_bands": (205, 7, [0.01], None, 0, False, False),
    "order2048": (None, 3, [0.002], None, 0, False, True),
}


def _audit_problem(oracle, name):
    """(problem whose families stand in the order of their largest count, indices of its edge families, parameters)."""
    max_count, n_taxa, lambdas, mus, clade, gamma, _ = AUDIT[name]
    lambdas = np.array(lambdas)
    strict = name != "order257_broad_bands"
    if max_count is None:
        # order 2048 through explicit sizes, one column tile: small families and families near the top (2047 is the last count
        # the tables hold) with the rows between them left to the far tails of both, families whose tips agree and families
        # whose tips lie far apart
        rng = np.random.default_rng(11)
        size = np.r_[np.linspace(3, 300, 20).astype(np.int64), np.linspace(1700, 2040, 70).astype(np.int64), 2047, 2047, 2000, 1950, 1900, 1850, 1800, 1750]
        far = np.r_[np.zeros(90, dtype=np.int64), 0, 300, 200, 500, 150, 400, 100, 250]
        rows = [{"A": int(s), "B": int(max(1, s - d - rng.integers(0, 3))), "C": int(max(1, s - rng.integers(0, 5)))} for s, d in zip(size, far)]
        pb = _explicit_problem("((A:7.25,B:23.904):61.337,C:9.75);", rows, 2047, 2047)
        assert pb.matrix_size == 2048 and pb.n_families <= 128
        pb, _ = R.with_rows(pb, np.zeros((0, 3), dtype=np.int32), sort=True)
        return pb, np.arange(0), P.Params(lambdas=lambdas, prior=P.prior_uniform(2047))
    pb0, _ = synth.make_problem(n_taxa=n_taxa, n_families=N_ORDINARY if strict else 260, max_count=max_count, lam_sim=0.003, seed=5, root_cap=max_count // 2,
                                lambda_clade_min=clade)
    assert pb0.matrix_size == (751 if max_count == 600 else 257) and pb0.n_lambdas == len(lambdas)
    prior = P.prior_uniform(pb0.max_root_family_size)
    pr = P.Params(lambdas=lambdas, prior=prior)
    if gamma:
        pr.cat_probs, pr.multipliers = oracle.discrete_gamma(2, R.ALPHA)
    # (with death rates the edge families are those of the same lambdas at lambda = mu, which is what the oracle computes; at
    # lambda = 0.01 no family gets near the edge and the least likely ones there are stand in)
    pb, idx, _, n_first = R.edge_problem(oracle, pb0, pr, sort=True, strict=strict)
    assert 256 < pb.n_families <= 300
    if strict:                                               # the denormal ones have the third column tile to themselves
        assert N_ORDINARY + n_first == 256 and (idx == np.arange(N_ORDINARY, pb.n_families)).all()
    return pb, idx, pr


@gpu
@pytest.mark.parametrize("name", list(AUDIT))
def test_every_skipped_k_step_underflows_against_the_operands(capi, oracle, monkeypatch, name):
    """Contexts without dedup and subtree dedup, families in the order of their largest count: panel column f is family f at
    every node and column tile ct holds the families 128 ct .. 128 ct + 127 -- asserted first, from column_extents.  Per
    interior non-root node v and category k, with P = ctx.matrix(v, k), the DEVICE's matrix, and L_v the panel computed on the
    CPU from the device's matrices of the call: for every (tile, 16-row block b, k-step ks) inside the range of
    CAFE_NO_MAGSKIP=1 and outside the default context's,

        max P[s][c] (s in 16 b + 1 .. 16 b + 16, c in 4 ks .. 4 ks + 3)  x  max L_v[c][f] (same c, f in the tile)  <  2^-1077,

    so that the four products of an MFMA sum to under 2^-1075, half the smallest denormal.  Some skipped steps hold non-zero
    products.  panel_bounds(v, k)[ct, r] >= log2 of every entry of rows 4 r .. 4 r + 3 of tile ct, without tolerance; and
    the root panels of the two contexts have the same bits.

    Why panels computed on the CPU will do: a step is skipped only when matrix bound + panel bound < -1100; the panel bound is
    at least -1050 inside the extent, so the matrix factor is below 2^-50; an entry computed on the CPU exceeds the device's by
    a few ulps plus a few times 2^-1074 at the most, which, times 2^-50, cannot carry a product over the 23 bits between
    2^-1100 and 2^-1077."""
    pb, edge, pr = _audit_problem(oracle, name)
    mus, must_skip = AUDIT[name][3], AUDIT[name][6]
    F, M, K = pb.n_families, pb.max_family_size, _categories(pr)
    n_tiles = (F + 127) // 128
    assert n_tiles == (1 if name == "order2048" else 3)
    assert (np.diff(pb.counts.max(axis=1)) >= 0).all()       # (the order a context gives its columns)
    alpha = 0.9 if K > 1 else 1.0
    new_ctx = _ctx(capi, monkeypatch, pb, (), mus, plain=True)
    old_ctx = _ctx(capi, monkeypatch, pb, ("CAFE_NO_MAGSKIP",), mus, plain=True)
    v_new, v_old = new_ctx.score(pr, alpha=alpha, per_family=True), old_ctx.score(pr, alpha=alpha, per_family=True)
    assert new_ctx.stats()["n_chunks"] == 1
    nodes = R.interior_non_root(pb)
    totals = dict(skipped=0, nonzero=0, worst=-np.inf, bound_rows=0)
    failures = []
    for k in range(K):
        mats = {v: new_ctx.matrix(v, k) for v in range(pb.n_nodes) if pb.parent[v] >= 0}
        for v in mats:                                       # (both contexts multiply the same matrices)
            assert mats[v].tobytes() == old_ctx.matrix(v, k).tobytes()
        panels = R.cpu_panels(pb, mats, pb.counts)
        for v in nodes:                                      # column f is family f: the reference's own statement
            L, ext = panels[v], new_ctx.column_extents(v, k)
            assert L.shape == (M + 1, F) and ext.shape[0] == 128 * n_tiles
            rows = np.arange(M + 1)[:, None]
            assert not ((L > 0) & ((rows < ext[None, :F, 0]) | (rows > ext[None, :F, 1]))).any(), (v, k)
        for v in nodes:
            L = panels[v]
            bound = new_ctx.panel_bounds(v, k)
            assert bound.shape[0] == n_tiles and bound.shape[1] * 4 >= M + 1
            Lp = np.zeros((4 * bound.shape[1], 128 * n_tiles))
            Lp[:M + 1, :F] = L
            top = R._log2(Lp.reshape(bound.shape[1], 4, n_tiles, 128).max(axis=(1, 3))).T      # [tile][row step]
            assert (bound >= top).all(), (v, k, np.argwhere(bound < top)[:4])
            assert (bound[np.isfinite(top)] >= -1060).all()
            totals["bound_rows"] += int(np.isfinite(top).sum())
            new, old = new_ctx.k_ranges(v, k), old_ctx.k_ranges(v, k)
            assert new.shape[0] == n_tiles
            n_skipped, n_nonzero, worst, where = R.audit_skipped_steps(mats[v], L, M, new, old)
            totals["skipped"] += n_skipped
            totals["nonzero"] += n_nonzero
            totals["worst"] = max(totals["worst"], worst)
            if not worst < R.SKIP_LOG2:
                failures.append((v, k, where, worst))
    print(name, "skipped k-steps: %(skipped)d, with a non-zero product: %(nonzero)d, largest log2 of a skipped product: %(worst).2f, "
          "bounds checked: %(bound_rows)d" % totals)
    assert not failures, failures[:8]
    assert totals["bound_rows"] > 100
    if must_skip:
        assert totals["nonzero"] > 0 and new_ctx.issued_flops() < old_ctx.issued_flops()
    _same(v_new, v_old)
    assert _root_panels(new_ctx, pb, pr).tobytes() == _root_panels(old_ctx, pb, pr).tobytes()
    new_ctx.close()
    old_ctx.close()


# ------------------------------------------------------------------ 3. the tables follow the call
def _fresh_answer(capi, monkeypatch, pb, run, pr):
    """What a fresh CAFE_NO_MAGSKIP=1 context that sees only this call answers: (result of run, root panels)."""
    ctx = _ctx(capi, monkeypatch, pb, ("CAFE_NO_MAGSKIP",))
    out = run(ctx)
    roots = _root_panels(ctx, pb, pr)
    ctx.close()
    return out, roots


def _equal_bytes(a, b):
    if isinstance(a, tuple):
        _same(a, b)
    else:
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


@gpu
def test_the_tables_are_those_of_the_call_not_of_the_one_before(capi, oracle, monkeypatch):
    """One default context at order 257 through a gamma call, a base call with other rates, root_max, the sum rule, back to the
    gamma call, and captured graphs replayed with two rate vectors in turn: after every step the result and the root panels
    have the bits of a fresh CAFE_NO_MAGSKIP=1 context given that call alone, and every call enqueued launch by launch issues
    fewer flops than it has products without an exact zero."""
    pb = _problem(205)
    assert pb.matrix_size == 257
    ctx = _ctx(capi, monkeypatch, pb)
    gamma, base = _params(oracle, pb, 0.002, True), _params(oracle, pb, 0.0007, False)
    score = lambda pr, alpha: (lambda c: c.score(pr, alpha=alpha, per_family=True))
    steps = [("gamma", score(gamma, 0.9), gamma, None),
             ("base, other rates", score(base, 1.0), base, None),
             ("root_max", lambda c: c.root_max(np.array([0.004])), base, None),
             ("sum rule", score(base, 1.0), base, "sum"),
             ("sum rule, gamma", score(gamma, 0.9), gamma, "sum"),
             ("max rule again", score(_params(oracle, pb, 0.004, False), 1.0), base, "max")]
    for label, run, pr, rule in steps:
        if rule:
            ctx.set_root_rule(rule)
        got = run(ctx)
        issued, executed = ctx.issued_flops(), ctx.executed_flops()
        roots = _root_panels(ctx, pb, pr)

        def fresh_run(c):
            if rule:
                c.set_root_rule(rule)
            return run(c)
        want, want_roots = _fresh_answer(capi, monkeypatch, pb, fresh_run, pr)
        print(label, "issued", issued, "without an exact zero", executed)
        _equal_bytes(got, want)
        assert roots.any() and roots.tobytes() == want_roots.tobytes(), label
        assert issued < executed, label
    ctx.set_graphs(True)
    for lam in (0.0007, 0.004, 0.0007):                      # the first call captures, the others replay with new rates
        pr = _params(oracle, pb, lam, True)
        run = score(pr, 0.9)
        got, roots = run(ctx), _root_panels(ctx, pb, pr)
        want, want_roots = _fresh_answer(capi, monkeypatch, pb, run, pr)
        _equal_bytes(got, want)
        assert roots.tobytes() == want_roots.tobytes(), lam
    ctx.close()


@gpu
def test_an_error_model_call_falls_back_and_the_next_plain_call_skips_again(capi, oracle, monkeypatch):
    """A context is created with or without an error model, and every scorer call of one that has it falls back to the exact
    extents; its plain call is root_max, which reads no error model.  Error-model call, root_max, error-model call with other
    rates, root_max with other rates: the bits of a fresh CAFE_NO_MAGSKIP=1 context every time; issued == executed flops in
    the error-model calls and issued < executed in the root_max calls between them."""
    pb = _problem(205, n_deviations=3)
    em = P.error_model_table(P.default_error_model(pb.max_family_size)[:1] + [[0.05, 0.9, 0.05]], pb.max_family_size)
    ctx = _ctx(capi, monkeypatch, pb)
    gamma, base = _params(oracle, pb, 0.002, True, em), _params(oracle, pb, 0.0007, False, em)
    steps = [("error model, gamma", lambda c: c.score(gamma, alpha=0.9, per_family=True), gamma, False),
             ("root_max", lambda c: c.root_max(np.array([0.0007])), base, True),
             ("error model, base", lambda c: c.score(base, alpha=1.0, per_family=True), base, False),
             ("root_max, other rates", lambda c: c.root_max(np.array([0.004])), base, True)]
    for label, run, pr, skips in steps:
        got = run(ctx)
        issued, executed = ctx.issued_flops(), ctx.executed_flops()
        roots = _root_panels(ctx, pb, pr)
        want, want_roots = _fresh_answer(capi, monkeypatch, pb, run, pr)
        print(label, "issued", issued, "without an exact zero", executed)
        _equal_bytes(got, want)
        assert roots.any() and roots.tobytes() == want_roots.tobytes(), label
        assert (issued < executed) if skips else (issued == executed), label
    ctx.close()
