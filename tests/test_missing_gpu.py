"""Missing cells on the GPU (CAFE_FLAG_MISSING_COUNTS): the scorer path, the per-family kernel, cafe_leaf_predictive and the
refusals, on the tables of tests/missing_ref.py (tests/test_missing_model.py shows what those tables can tell apart and where
their missing cells sit).

Reference: the numpy prune of missing_ref.py on the matrices the context's own call built (marginal_ref.context_matrices) -- the
matrices are K1's, pinned elsewhere; what is under test is every reader of a count.  Tolerance 1e-10 relative, the GPU parity
tests' value; "the same bits" is == on the doubles.  Matrix orders 41 (no extents) and 300 (extents, magnitude skip, K ranges).
"""
import dataclasses

import numpy as np
import pytest

import marginal_ref as MR
import missing_ref as MS
from cafexp_amd import problem as P
from test_leaf_predictive_shapes import C_BOUND
from test_per_family_shapes import TREE3, WIDTHS, sizes, width

pytestmark = pytest.mark.gpu
REL = 1e-10
ORDERS = (41, 300)


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _ctx(capi, monkeypatch, pb, K=1, env=(), **kw):
    for name in ("CAFE_NO_CHERRY_SWAP", "CAFE_NO_KSKIP", "CAFE_NO_MAGSKIP", "CAFE_NO_ASM_SKIP"):
        monkeypatch.delenv(name, raising=False)
    for name in env:
        monkeypatch.setenv(name, "1")
    try:
        return capi.Context(pb, max_categories=K, **kw)
    finally:
        for name in env:
            monkeypatch.delenv(name, raising=False)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _K(pr):
    return 1 if pr.multipliers is None else len(pr.multipliers)


def _score(ctx, pr):
    total, res = ctx.score(pr, per_family=True)
    return total, res["family_lnl"]


_stats = {}          # (order, model) -> schedule counters and diagnostics of the contexts of the parity test


# ------------------------------------------------------------------------------------------------ 2. scorer against numpy
@pytest.mark.parametrize("model", MS.MODELS)
@pytest.mark.parametrize("order", ORDERS)
def test_the_scorer_matches_the_numpy_prune(capi, monkeypatch, order, model):
    pb = MS.problem(order, model)
    pr = MS.params(pb, model)
    ctx = _ctx(capi, monkeypatch, pb, K=_K(pr))
    try:
        ctx.set_death_rates(MS.death_rates(model))
        for rule in ("max", "sum"):
            ctx.set_root_rule(rule)
            total, lnl = _score(ctx, pr)
            mats = MR.context_matrices(ctx, pb, _K(pr))
            want = MS.family_lnl(pb, pr, mats, root_rule=rule)
            worst = MS.rel(lnl, want, MS.all_missing(pb))
            print("order %d %s %s: worst relative difference %.3g over %d families; -lnL %.12g" % (order, model, rule, worst, len(want), total))
            assert np.isfinite(want).all() and worst <= REL
            assert abs(total + want.sum()) <= REL * abs(want.sum())
            # a family and its duplicate, the same bits
            n = MS.N_DISTINCT + 1
            for i, src in enumerate(MS.SOURCE_OF_DUPLICATES):
                assert _same(lnl[n + 2 + i], lnl[src])
        st = ctx.stats()
        _stats[(order, model)] = dict(st, leaf_transposes=ctx.leaf_transposes())
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 3. coverage
def test_the_contexts_reach_every_ported_path(capi, monkeypatch):
    if len(_stats) < len(ORDERS) * len(MS.MODELS):          # (run on its own: the counters are fixed at cafe_create)
        for order in ORDERS:
            for model in MS.MODELS:
                pb = MS.problem(order, model)
                ctx = _ctx(capi, monkeypatch, pb, K=_K(MS.params(pb, model)))
                _stats[(order, model)] = dict(ctx.stats(), leaf_transposes=ctx.leaf_transposes())
                ctx.close()
    for key, st in sorted(_stats.items()):
        print(key, {k: st[k] for k in ("n_leaf_passes", "n_assemble_passes", "n_gather_epilogues", "n_unique_families")}, st["leaf_transposes"])
        assert st["n_leaf_passes"] > 0
        # the planner keeps a table with missing cells off the transposed leaf copies: none are made
        assert st["leaf_transposes"] == (0, False)
    assert sum(st["n_assemble_passes"] for st in _stats.values()) > 0
    # n_gather_epilogues counts the K2 launches that fold a sibling's GATHERED FACTOR into their epilogue: they read no count
    # and are not changed; K2's leaf epilogues, which do, are what the planner routes such a table around (printed above)


def test_extents_and_bounds_with_a_missing_leaf_child_at_order_300(capi, monkeypatch):
    """One column per family at every node (no subtree sharing), so that column f of every panel is family f: the exact-zero
    intervals hold every non-zero of the numpy panel and are not trivial, the magnitude bounds dominate the numpy values, and the
    K ranges of the branch above a node with a missing leaf child are cut."""
    order = 300
    pb = MS.problem(order, "base")
    pr = MS.params(pb, "base")
    U = MS.N_DISTINCT + 3                                    # distinct families = columns: family f is column f (root_columns)
    assert np.array_equal(MS.root_columns(pb.counts)[:U], np.arange(U))
    ctx = _ctx(capi, monkeypatch, pb, subtree_dedup=False)
    try:
        _, lnl = _score(ctx, pr)
        mats = MR.context_matrices(ctx, pb, 1)
        B, _ = MS.up(pb, pr, mats[0])
        assert MS.rel(lnl, MS.family_lnl(pb, pr, mats), MS.all_missing(pb)) <= REL
        names = pb.node_names
        x = names.index("ABG")                              # children: the cherry and the leaf G
        t = names.index("CDE")                              # the polytomy
        g_missing = pb.counts[:, pb.taxa.index("G")] < 0
        for v in (x, t):
            ext = ctx.column_extents(v, 0)[:U]
            Bv = B[v][:, :U]
            rows = np.arange(Bv.shape[0])[:, None]
            outside = (rows < ext[:, 0][None, :]) | (rows > ext[:, 1][None, :])
            assert not (Bv[outside] != 0.0).any()            # exact: nothing non-zero lies outside
            assert outside[:, 1:].any() and (ext[1:, 1] >= ext[1:, 0]).all()     # and not trivial
            bounds = ctx.panel_bounds(v, 0)                  # [tiles][row steps], log2
            # (-inf marks the row steps outside a tile's hull; a tile that holds a padding column or the all-missing family has none)
            print("node %s: bounds of %d tiles x %d row steps, %d outside a hull, range %.1f .. %.1f" % (
                names[v], bounds.shape[0], bounds.shape[1], int(np.isneginf(bounds).sum()), bounds[np.isfinite(bounds)].min(), bounds.max()))
            assert np.isfinite(bounds).any() and bounds[np.isfinite(bounds)].min() < -1.0        # not the trivial bound (0: a product of probabilities) either
            for tile in range(bounds.shape[0]):
                cols = slice(128 * tile, min(128 * (tile + 1), U))
                for r in range(bounds.shape[1]):
                    blk = Bv[4 * r:4 * r + 4, cols]
                    if blk.size and blk.max() > 0:
                        assert np.log2(blk.max()) <= bounds[tile, r] + 1e-9, (names[v], tile, r)
        # family 0 (every cell missing): both panels are 1 in every row, the interval is everything
        e0 = ctx.column_extents(x, 0)[0]
        print("node ABG, the family with every cell missing: rows", tuple(e0))
        assert e0[0] == 0 and e0[1] >= pb.max_family_size - 16 and np.all(B[names.index("AB")][:, 0] == 1.0)
        assert g_missing[[127, 128, 255, 256]].all()
        kr = ctx.k_ranges(x, 0)                              # [tiles][blocks][2]
        full = (pb.max_family_size + 1 + 3) // 4 - 1
        some = kr[..., 1] >= kr[..., 0]
        assert some.any() and ((kr[..., 0][some] > 0) | (kr[..., 1][some] < full)).any()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. drop a leaf
@pytest.mark.parametrize("order", ORDERS)
def test_a_leaf_missing_everywhere_is_the_tree_without_it(capi, monkeypatch, order):
    full = MS.table(order, blank=False)[1:]
    e = MS.SPECIES.index("E")
    blanked = full.copy()
    blanked[:, e] = MS.MISSING
    pb = MS.problem(order, "base", counts=blanked)
    small = MS.problem(order, "base", counts=np.delete(full, e, axis=1), newick=MS.NEWICK.replace(",E:3", ""),
                       species=[s for s in MS.SPECIES if s != "E"])
    assert pb.missing_counts and not small.missing_counts and small.n_taxa == pb.n_taxa - 1
    pr = MS.params(pb, "base")
    a, b = _ctx(capi, monkeypatch, pb), _ctx(capi, monkeypatch, small)
    try:
        (ta, la), (tb, lb) = _score(a, pr), _score(b, pr)
        worst = MS.rel(la, lb)
        print("order %d: worst relative difference to the tree without the leaf %.3g" % (order, worst))
        assert worst <= 1e-12 and abs(ta - tb) <= 1e-12 * abs(tb)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 5. bit identity
def test_what_only_changes_the_work_changes_no_bit(capi, monkeypatch):
    order = 300
    pb = MS.problem(order, "gamma")
    pr = MS.params(pb, "gamma")
    K = _K(pr)

    def run(**kw):
        ctx = _ctx(capi, monkeypatch, pb, K=K, **kw)
        try:
            total, res = ctx.score(pr, per_family=True)
            return total, res, ctx.stats()
        finally:
            ctx.close()

    total, res, st = run()
    assert st["n_chunks"] == 1
    cases = {"no_dedup": dict(dedup=False), "no_subtree_dedup": dict(subtree_dedup=False), "no_cherry_swap": dict(env=("CAFE_NO_CHERRY_SWAP",)),
             "no_kskip": dict(env=("CAFE_NO_KSKIP",)), "no_magskip": dict(env=("CAFE_NO_MAGSKIP",)), "no_asm_skip": dict(env=("CAFE_NO_ASM_SKIP",)),
             "chunks": None}
    for name, kw in cases.items():
        if name == "chunks":                                # the largest of these limits that cuts the columns into several chunks
            for mb in (16, 12, 8, 6, 4):
                t2, r2, s2 = run(workspace_limit=mb << 20)
                if s2["n_chunks"] >= 2:
                    break
        else:
            t2, r2, s2 = run(**kw)
        print(name, t2, "chunks", s2["n_chunks"], "columns", s2["n_unique_families"])
        if name == "chunks":
            assert s2["n_chunks"] >= 2
        for key in ("family_lnl", "family_likelihood", "category_likelihood", "failed"):
            assert _same(res[key], r2[key]) if res[key].dtype == np.float64 else np.array_equal(res[key], r2[key]), (name, key)
        if name not in ("no_dedup", "chunks"):              # (the final sum runs over other columns, or in other blocks, there)
            assert _same(total, t2), name
        else:
            assert abs(total - t2) <= 1e-13 * abs(total), name
    # a two-shard plan on one GPU: cafe_shard_plan's partition, one context per shard on device 0, the shards' sums added
    plan = capi.shard_plan(pb, 2, K)
    assert sorted(np.concatenate(plan).tolist()) == list(range(pb.n_families)) and min(len(x) for x in plan) > 50
    parts = 0.0
    for fam in plan:
        shard = dataclasses.replace(pb, counts=np.ascontiguousarray(pb.counts[fam]), family_ids=[pb.family_ids[i] for i in fam],
                                    missing_counts=True)
        ctx = _ctx(capi, monkeypatch, shard, K=K)
        try:
            t2, r2 = ctx.score(pr, per_family=True)
        finally:
            ctx.close()
        parts += t2
        for key in ("family_lnl", "family_likelihood", "category_likelihood"):
            assert _same(res[key][fam], r2[key]), ("shard", key)
    assert abs(total - parts) <= 1e-13 * abs(total)
    sh = capi.Sharded(pb, [0], max_categories=K)            # and cafe_create_sharded / cafe_sharded_score pass the flag on
    try:
        t2, r2 = sh.score(pr, per_family=True)
        assert abs(total - t2) <= 1e-13 * abs(total)
        for key in ("family_lnl", "family_likelihood", "category_likelihood"):
            assert _same(res[key], r2[key]), ("sharded", key)
    finally:
        sh.close()
    n = MS.N_DISTINCT + 1
    for i, src in enumerate(MS.SOURCE_OF_DUPLICATES):
        assert _same(res["family_lnl"][n + 2 + i], res["family_lnl"][src])


# ------------------------------------------------------------------------------------------------ 6. the flag without a missing cell
@pytest.mark.parametrize("order", ORDERS)
def test_the_flag_on_a_table_without_missing_cells_changes_nothing(capi, monkeypatch, order):
    pb = MS.problem(order, "error3", counts=MS.table(order, blank=False))
    assert not pb.missing_counts
    pr = MS.params(pb, "error3")
    out = []
    for flagged in (False, True):
        ctx = _ctx(capi, monkeypatch, MS.with_flag(pb, flagged))
        try:
            total, lnl = _score(ctx, pr)
            st = ctx.stats()
            out.append((total, lnl, {k: st[k] for k in ("n_assemble_passes", "n_gather_epilogues", "n_leaf_passes", "n_unique_families",
                                                         "n_chunks", "gemm_launches", "n_matrices", "panel_bytes")}, ctx.leaf_transposes()[0]))
            if flagged:                                     # and nothing is refused
                ctx.marginal_reconstruct(pr)
                ctx.root_max(pr.lambdas)
        finally:
            ctx.close()
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1]) and out[0][2] == out[1][2] and out[0][3] == out[1][3]


def test_a_negative_count_is_still_rejected(capi):
    pb = MS.problem(41, "base")
    with pytest.raises(capi.CafeError, match=r"has a count outside \[0, 40\]"):
        capi.Context(MS.with_flag(pb, False))               # -1 without the flag: as before, the same message
    bad = dataclasses.replace(pb, counts=np.where(pb.counts == -1, -2, pb.counts).astype(np.int32))
    with pytest.raises(capi.CafeError, match=r"has a count outside \[0, 40\]"):
        capi.Context(bad)                                   # any other negative value with it


# ------------------------------------------------------------------------------------------------ 7. the per-family kernel
PF_ORDERS = [3, 129, 257, 385, 513, 641, 769, 897, 1025, 1281, 1537, 2048]


def test_the_per_family_orders_hit_every_width_once():
    assert sorted(width(n) for n in PF_ORDERS) == WIDTHS


# (the error model's taps are one code path for every width: checked at a narrow and at the widest one)
@pytest.mark.parametrize("n,error", [(n, False) for n in PF_ORDERS] + [(129, True), (2048, True)])
def test_the_per_family_kernel_agrees_with_the_scorer(capi, monkeypatch, n, error):
    M, R = sizes(n)
    q = max(1, n // 4)
    rows = [(3, 5, 2), (q, -1, q + q // 16), (-1, 1, 1), (40, 44, -1), (-1, -1, 2), (-1, -1, -1), (0, 1, -1)]
    counts = np.array([[min(c, M) for c in r] for r in rows], dtype=np.int32)
    pb = P.build_problem(P.parse_newick(TREE3), ["A", "B", "C"], ["f%d" % i for i in range(len(rows))], counts, root_filter=False,
                         max_family_size=M, max_root_family_size=R, n_deviations=3 if error else 0, missing_tokens=("NA",))
    assert pb.matrix_size == n and pb.missing_counts
    lam, mu = 0.0051, 0.00408
    pr = P.Params(lambdas=np.array([lam]), prior=P.prior_uniform(R), error_model=MS.error_model(M, 3) if error else None)
    ctx = _ctx(capi, monkeypatch, pb)
    try:
        fam = np.arange(pb.n_families)
        want = _score(ctx, pr)[1]
        got = ctx.score_per_family(pr, fam, np.full(len(fam), lam))
        print("order %d: per-family against the scorer %.3g" % (n, MS.rel(got, want, MS.all_missing(pb))))
        assert MS.rel(got, want, MS.all_missing(pb)) <= REL and np.isfinite(want).all()
        ctx.set_death_rates(np.array([mu]))
        want = _score(ctx, pr)[1]
        ctx.set_death_rates(None)
        got = ctx.score_per_family_lm(pr, fam, np.full(len(fam), lam), np.full(len(fam), mu))
        assert MS.rel(got, want, MS.all_missing(pb)) <= REL
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 8. imputation
@pytest.mark.parametrize("model", ["gamma", "error3"])
@pytest.mark.parametrize("order", ORDERS)
def test_leaf_predictive_imputes_a_missing_cell(capi, monkeypatch, order, model):
    counts, full = MS.table(order)[:140], MS.table(order, blank=False)[:140]
    pb, pb_full = MS.problem(order, model, counts=counts), MS.problem(order, model, counts=full)
    other = np.where(counts < 0, np.minimum(full + 3, MS.SHAPES[order][2]), counts).astype(np.int32)      # the blanked cells filled otherwise
    pb_other = MS.problem(order, model, counts=other)
    pr = MS.params(pb, model)
    K = _K(pr)
    res = {}
    for name, p in (("missing", pb), ("full", pb_full), ("other", pb_other)):
        ctx = _ctx(capi, monkeypatch, p, K=K)
        try:
            res[name] = ctx.leaf_predictive(pr)
            if name == "missing":
                mats = MR.context_matrices(ctx, pb, K)
                ctx.set_root_rule("sum")
                evidence = _score(ctx, pr)[1]
        finally:
            ctx.close()
    got = res["missing"]
    miss = pb.counts < 0                                     # (the outputs' columns are the problem's taxa, in tree order)
    one = miss.sum(axis=1) == 1                              # families with exactly one missing cell: filling it gives the same other cells
    cell = miss & one[:, None]
    assert cell.sum() >= 20
    for key in ("mean", "sd"):
        for name in ("full", "other"):                       # the promise of the header: they do not depend on x, not in the last bit
            assert _same(got[key][cell], res[name][key][cell]), (key, name)
        assert np.isfinite(got[key][miss]).all()
    for key in ("p_below", "p_obs", "p_above"):
        assert np.isnan(got[key][miss]).all() and np.isfinite(got[key][~miss]).all()
    ref = MS.predictive(pb, pr, mats)
    for key in ("mean", "sd", "p_below", "p_obs", "p_above"):
        ok = ~np.isnan(ref[key])
        assert np.array_equal(np.isnan(got[key]), ~ok), key
        if key == "sd":                                      # a difference of moments: held to its cancellation factor below
            continue
        worst = float((np.abs(got[key][ok] - ref[key][ok]) / (1e-12 + REL * np.abs(ref[key][ok]))).max())
        print("order %d %s %s: worst |got - ref| / (1e-12 + 1e-10 |ref|) = %.3g" % (order, model, key, worst))
        assert worst <= 1.0, key
    assert MS.rel(got["log_evidence"], ref["log_evidence"], MS.all_missing(pb)) <= REL
    assert MS.rel(got["log_evidence"], evidence, MS.all_missing(pb)) <= REL and not got["failed"].any()
    # sd: the project's rule for this call (leaf_predictive_ref.close): 1e-10 times the cancellation factor of the kernel's
    # formula, 1 + mean^2 / var (it takes its moments about 0 so that they cannot depend on x, predictive.hip), capped at the
    # existing predictive tests' C_BOUND -- a badly cancelled sd cannot pass
    ok = ~np.isnan(ref["sd"]) & (ref["sd"] > 0)
    cancel = np.minimum(1 + ref["mean"][ok] ** 2 / ref["sd"][ok] ** 2, C_BOUND)
    print("order %d %s: sd cancellation factors up to %.3g (cap %g)" % (order, model, float((1 + ref["mean"][ok] ** 2 / ref["sd"][ok] ** 2).max()), C_BOUND))
    assert np.all(np.abs(got["sd"][ok] - ref["sd"][ok]) <= 1e-12 + REL * cancel * ref["sd"][ok])
    zero = ~np.isnan(ref["sd"]) & (ref["sd"] == 0)
    assert np.all(got["sd"][zero] <= 1e-12)


# ------------------------------------------------------------------------------------------------ 2b. the other scorer entries
def test_root_max_root_posterior_and_score_partial_accept_missing_cells(capi, monkeypatch):
    """cafe_root_max against the numpy prune (max_j L_j, no prior); cafe_root_posterior's log_evidence against the sum-rule scorer
    and its mean against numpy; cafe_score_partial + cafe_finish_partial against cafe_score, the same bits."""
    import torch
    order = 300
    pb = MS.problem(order, "base")
    pr = MS.params(pb, "base")
    ctx = _ctx(capi, monkeypatch, pb)
    try:
        total, lnl = _score(ctx, pr)
        mats = MR.context_matrices(ctx, pb, 1)
        R = pb.max_root_family_size
        inside = MS.up(pb, pr, mats[0])[0][MR.root_of(pb)][1:R + 1]          # [R][F]
        got = ctx.root_max(pr.lambdas)
        assert MS.rel(got, inside.max(axis=0)) <= REL
        ctx.set_root_rule("sum")
        evidence = _score(ctx, pr)[1]
        ctx.set_root_rule("max")
        post = ctx.root_posterior(pr)
        assert MS.rel(post["log_evidence"], evidence, MS.all_missing(pb)) <= REL and not post["failed"].any()
        prior = np.asarray(pr.prior, dtype=np.float64)[:R, None]
        w = inside * prior
        assert MS.rel(post["mean"], (np.arange(1, R + 1)[:, None] * w).sum(axis=0) / w.sum(axis=0)) <= REL
        pair = torch.zeros(2, dtype=torch.float64, device="cuda:0")
        ctx.score_partial(pr, pair.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert _same(ctx.finish(pair.cpu().numpy()), total)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_the_other_calls_refuse_cleanly_and_leave_the_context_usable(capi, monkeypatch):
    order = 41
    pb = MS.problem(order, "base")
    pr = MS.params(pb, "base")
    sizes_ = np.zeros((pb.n_families, pb.n_nodes), dtype=np.int32)
    calls = {
        "cafe_pvalues": lambda c: c.pvalues(pr.lambdas, n_simulations=10),
        "cafe_reconstruct": lambda c: c.reconstruct(pr.lambdas, np.ones(pb.max_root_family_size + 1, dtype=np.float32)),
        "cafe_branch_probabilities": lambda c: c.branch_probabilities(pr.lambdas, sizes_),
        "cafe_marginal_reconstruct": lambda c: c.marginal_reconstruct(pr),
        "cafe_sample_histories": lambda c: c.sample_histories(pr, 2, 1),
        "cafe_score_gradient": lambda c: c.score_gradient(pr),
        "cafe_branch_scores": lambda c: c.branch_scores(pr),
        "cafe_expected_events": lambda c: c.expected_events(pr),
    }
    ctx = _ctx(capi, monkeypatch, pb)
    try:
        before = _score(ctx, pr)
        for name, call in calls.items():
            with pytest.raises(capi.CafeError, match=r"code 4: %s: the table has missing cells" % name):
                call(ctx)
            after = _score(ctx, pr)
            assert _same(before[0], after[0]) and _same(before[1], after[1]), name
    finally:
        ctx.close()
    ok = MS.problem(order, "base", counts=MS.table(order, blank=False)[1:])
    ctx = _ctx(capi, monkeypatch, MS.with_flag(ok, True))
    try:
        sizes_ = np.zeros((ok.n_families, ok.n_nodes), dtype=np.int32)
        for name, call in calls.items():
            call(ctx)                                       # the flag without a missing cell: every call goes through
    finally:
        ctx.close()
