"""cafe_branch_change on the device against tests/branch_change_ref.py fed the matrices the call itself built
(marginal_ref.context_matrices), on the seven-taxon tables of branch_change_ref (at most 312 families; what they can tell is
shown on the CPU by tests/test_branch_change_model.py).

Tolerance (branch_change_ref.compare): pmf and tails 1e-10 relative -- the project's GPU parity value; every entry is a sum of
non-negative products, so its relative error is of order (terms) x eps -- with an entry whose reference value is below 1e-250
checked absolutely against 1e-250, the level the magnitude audit treats as the edge of fp64; mean to 1e-10 of max(1, the larger
of the two node means), since it is a difference of two means; mode, lo and hi exactly, except where the reference's own CDF lies
within 1e-9 of the threshold or its two best masses within 1e-9 relative.

Matrix orders 41 (no extents), 300 (extents; M = 299, R = 250) and 41 with R > M.  D: 0 (the tails are then the marginal
reconstruction's p_decrease and p_increase), 1, 3 and 4 (2 D + 1 = 7 and 9: either side of the band kernel's block of 8
accumulators), 7 and 8 (15 and 17), and 40 at order 41 (no tail is left: exactly 0.0)."""
import json
import os
import subprocess

import numpy as np
import pytest

import branch_change_ref as BR
import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import DATA, read, table

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
kBandD, kBN = 8, 128                                        # branch_change.hip's accumulator block, the column tile
D_SMALL = (0, 1, 3, 4, 7, 8, 40)
D_LARGE = (0, 4, 10, 32)


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _K(pr):
    return 1 if pr.multipliers is None else len(pr.multipliers)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _invariants(got, D):
    ok = got["failed"] == 0
    band = got["pmf"][ok]
    live = ~np.isnan(got["below"][ok])
    total = np.nansum(band, axis=2) + got["below"][ok] + got["above"][ok]
    assert np.all(np.abs(total[live] - 1.0) <= 1e-10)
    for key in ("mode", "lo", "hi"):
        v = got[key][ok][live]
        assert np.all(np.abs(v) <= D + (0 if key == "mode" else 1)), key
    assert np.all(got["lo"][ok][live] <= got["hi"][ok][live])


def _run(capi, pb, pr, label, Ds, level=0.95, mus=None, **ctx_args):
    """One context, one call per D, each compared with the reference's one pass on the matrices the first call built.
    -> {D: got}, the reference's states, the context (open: the caller closes it)."""
    K = _K(pr)
    ctx = capi.Context(pb, max_categories=K, **ctx_args)
    try:
        if mus is not None:
            ctx.set_death_rates(mus)
        alpha = 0.7 if K > 1 else 1.0
        out, states = {}, None
        root = MR.root_of(pb)
        for D in Ds:
            got = ctx.branch_change(pr, max_change=D, level=level, alpha=alpha)
            if states is None:
                states = BR.diagonals(pb, pr, MR.context_matrices(ctx, pb, K))
            ref = BR.summarise(pb, states, D, level)
            share = BR.compare(got, ref, "%s D %d" % (label, D))
            print("%s D %d: excusable share %.4f" % (label, D, share))
            _invariants(got, D)
            assert got["pmf"].shape == (pb.n_families, pb.n_nodes, 2 * D + 1)
            assert np.all(np.isnan(got["pmf"][:, root])) and np.all(np.isnan(got["mean"][:, root]))
            assert np.all(got["mode"][:, root] == capi.CAFE_CHANGE_NONE) and np.all(got["lo"][:, root] == capi.CAFE_CHANGE_NONE)
            out[D] = got
    except BaseException:
        ctx.close()
        raise
    return out, states, ctx


def _common_band_bits(out):
    """pmf bits on the common band of every pair of D, and the D-free outputs"""
    Ds = sorted(out)
    for a, b in zip(Ds, Ds[1:]):
        assert _same(out[a]["pmf"], out[b]["pmf"][:, :, b - a:b + a + 1]), (a, b)
        for key in ("mean", "log_evidence"):
            assert _same(out[a][key], out[b][key]), (a, b, key)


# ------------------------------------------------------------------------------------------------ 1. every D, three orders
def test_order_41_every_band_width_and_the_marginal_tails(capi):
    """Order 41, no extents, three column tiles with a partial last one: every D; D = 0 against cafe_marginal_reconstruct on the same
    context; D = 40 leaves no tail; pmf bits on the common band of every two D; identical families get identical rows."""
    pb = BR.problem(41)
    pr = BR.params(pb)
    out, _, ctx = _run(capi, pb, pr, "order 41 base", D_SMALL)
    try:
        assert ctx.stats()["n_unique_families"] == len(np.unique(pb.counts, axis=0)) > 2 * kBN
        mr = ctx.marginal_reconstruct(pr)
    finally:
        ctx.close()
    root = MR.root_of(pb)
    inner = [v for v in range(pb.n_nodes) if v != root]
    for mine, theirs in (("above", "p_increase"), ("below", "p_decrease")):
        g, r = out[0][mine][:, inner], mr[theirs][:, inner]
        assert np.all(np.abs(g - r) <= 1e-10 * np.abs(r) + 1e-250), mine
    assert _same(out[0]["log_evidence"], mr["log_evidence"])
    assert np.all(out[40]["below"][:, inner] == 0.0) and np.all(out[40]["above"][:, inner] == 0.0)
    _common_band_bits(out)
    assert {2 * D + 1 for D in D_SMALL} >= {kBandD - 1, kBandD + 1, 2 * kBandD - 1, 2 * kBandD + 1}      # either side of one block, of two
    _, first, inverse = np.unique(pb.counts, axis=0, return_index=True, return_inverse=True)
    twin = first[np.asarray(inverse).reshape(-1)]            # the first family with the same counts
    assert (twin != np.arange(pb.n_families)).sum() >= 7
    for key, val in out[4].items():
        assert np.array_equal(val, val[twin], equal_nan=True), key


def test_order_300_with_extents(capi):
    """Order 300 (M = 299, R = 250): K1 writes extents, so the band kernel skips blocks of i; the last block of 16 parent sizes is
    partial under the root (250 = 15 x 16 + 10) and below it (299 = 18 x 16 + 11)."""
    pb = BR.problem(300)
    pr = BR.params(pb)
    out, states, ctx = _run(capi, pb, pr, "order 300 base", D_LARGE)
    try:
        v = next(v for v in range(pb.n_nodes) if pb.leaf_taxon[v] < 0 and pb.parent[v] >= 0)
        ext, _ = ctx.extents(v)
    finally:
        ctx.close()
    assert np.any(ext[:, 0] > 0) or np.any(ext[:ext.shape[0] - 1, 1] < pb.max_family_size)       # some block's extent is narrower than the matrix
    _common_band_bits(out)
    assert min(st["Z"] for st in states) >= 1e-250
    inner = [v for v in range(pb.n_nodes) if v != MR.root_of(pb)]
    assert np.nanmax(out[10]["below"][:, inner]) > 0.5 and np.nanmax(out[10]["above"][:, inner]) > 0.5     # tails that matter
    assert np.any(out[10]["lo"][:, inner] == -11) and np.any(out[10]["hi"][:, inner] == 11)               # ... and clip intervals


def test_order_41_with_the_root_range_above_m(capi):
    pb = BR.root_above_problem()
    pr = P.Params(lambdas=np.array([0.012]), prior=P.prior_uniform(pb.max_root_family_size))
    out, _, ctx = _run(capi, pb, pr, "order 41 R > M", (0, 3, 4, 40), level=0.5)
    ctx.close()
    _common_band_bits(out)
    inner = [v for v in range(pb.n_nodes) if v != MR.root_of(pb)]
    assert np.all(out[40]["below"][:, inner] == 0.0) and np.all(out[40]["above"][:, inner] == 0.0)


# ------------------------------------------------------------------------------------------------ 2. models
@pytest.mark.parametrize("order", [41, 300])
@pytest.mark.parametrize("model", [m for m in BR.MODELS if m != "base"])
def test_models(capi, order, model):
    """Gamma K = 3, two lambdas, death rates, 3- and 5-tap error models (the leaf kernel's taps, counts 0 and near M included)."""
    pb = BR.problem(order, model)
    pr = BR.params(pb, model)
    out, _, ctx = _run(capi, pb, pr, "order %d %s" % (order, model), (1, 4) if order == 41 else (10,), mus=BR.death_rates(model))
    ctx.close()
    if pr.error_model is not None:                          # a leaf's change is no longer pinned to x - i: its band has several taps' mass
        leaves = np.where(pb.leaf_taxon >= 0)[0]
        D = max(out)
        assert np.any((out[D]["pmf"][:, leaves] > 1e-3).sum(axis=2) >= 3)


# ------------------------------------------------------------------------------------------------ 3. batches
def _per_col(pb, D):
    """branch_change_impl's own workspace formula: bytes per column"""
    n, nI, rows = pb.n_nodes, int((pb.leaf_taxon < 0).sum()), pb.matrix_size
    return (4 * nI * rows + 2 * rows + n * (2 * D + 3) + 1 + 2 * n) * 8 + 3 * n * 4


@pytest.mark.parametrize("model", ["base", "error3"])
def test_column_batches_change_no_bit(capi, model):
    """305 distinct families are 384 padded columns: one batch, 256 + 128 (the last one narrower than the workspace's stride) and
    three batches of 128 give the same bits in every output; so does switching the column dedup off (312 columns)."""
    pb = BR.problem(41, model)
    pr = BR.params(pb, model)
    D = 5
    ctx = capi.Context(pb)
    try:
        padded = -(-ctx.stats()["n_unique_families"] // kBN) * kBN
        want = ctx.branch_change(pr, max_change=D)
    finally:
        ctx.close()
    assert padded == 3 * kBN
    per_col = _per_col(pb, D)
    for cols, dedup in ((256, True), (128, True), (128, False)):
        limit = cols * per_col + per_col // 2
        assert limit // per_col // kBN * kBN == cols < padded
        ctx = capi.Context(pb, workspace_limit=limit, dedup=dedup)
        try:
            got = ctx.branch_change(pr, max_change=D)
        finally:
            ctx.close()
        assert got.keys() == want.keys()
        for key in want:
            same = _same(got[key], want[key]) if want[key].dtype == np.float64 else np.array_equal(got[key], want[key])
            assert same, (cols, dedup, key)


def test_one_partial_tile_and_no_pmf(capi):
    """40 families: one partial column tile.  pmf=False allocates no band on the host and changes nothing else."""
    full = BR.problem(41)
    rows = np.r_[0:20, 280:296, 308:312]
    pb = BR._tables().problem(41, "base", counts=BR.table(41)[rows])
    pr = BR.params(pb)
    out, _, ctx = _run(capi, pb, pr, "one partial tile", (3,))
    try:
        lean = ctx.branch_change(pr, max_change=3, pmf=False)
    finally:
        ctx.close()
    assert "pmf" not in lean
    for key in lean:
        assert np.array_equal(lean[key], out[3][key], equal_nan=True), key
    assert pb.n_families == 40 and full.n_nodes == pb.n_nodes


# ------------------------------------------------------------------------------------------------ 4. families and states
def test_a_failed_family_beside_good_ones(capi):
    """A's branch quantizes to t_q = 0: its matrix is e_0 in row 0 and zero below, so a family is possible only with A = 0 under an
    extinct parent, hence B = 0 too.  Every second family is made so; the others fail, in the same batch: NaN and CAFE_CHANGE_NONE on
    them only."""
    MS = BR._tables()
    counts = BR.table(41)[1:61].copy()
    counts[::2, :2] = 0                                      # columns A, B
    pb = MS.problem(41, "base", counts=counts, newick=MS.NEWICK.replace("A:3", "A:0.0004"))
    pr = BR.params(pb)
    possible = (counts[:, 0] == 0) & (counts[:, 1] == 0)
    assert possible.sum() >= 25 and (~possible).sum() >= 25
    ctx = capi.Context(pb)
    try:
        got = ctx.branch_change(pr, max_change=4)
        ref = BR.change(pb, pr, MR.context_matrices(ctx, pb, 1), 4, 0.95)
    finally:
        ctx.close()
    assert np.array_equal(ref["failed"] == 0, possible)
    BR.compare(got, ref, "t_q = 0")
    for key in ("pmf", "below", "above", "mean", "log_evidence"):
        assert np.all(np.isnan(got[key][~possible])), key
    for key in ("mode", "lo", "hi"):
        assert np.all(got[key][~possible] == capi.CAFE_CHANGE_NONE), key
    root = MR.root_of(pb)
    inner = [v for v in range(pb.n_nodes) if v != root]
    assert np.all(np.isfinite(got["pmf"][possible][:, inner])) and np.all(np.isfinite(got["mean"][possible][:, inner]))
    assert np.all(got["mode"][possible][:, inner] != capi.CAFE_CHANGE_NONE)
    ab = int(pb.parent[int(np.where(pb.leaf_taxon == pb.taxa.index("A"))[0][0])])
    assert np.all(got["hi"][possible, ab] <= 0)               # the parent of A is extinct: no branch into it grows


def test_no_side_effect_on_the_scorer(capi):
    pb = BR.problem(41, "gamma")
    pr = BR.params(pb, "gamma")
    ctx = capi.Context(pb, max_categories=3)
    try:
        before, fam0 = ctx.score(pr, alpha=0.7, per_family=True)
        ctx.branch_change(pr, max_change=6, alpha=0.7)
        after, fam1 = ctx.score(pr, alpha=0.7, per_family=True)
    finally:
        ctx.close()
    assert np.float64(before).tobytes() == np.float64(after).tobytes()
    for key in fam0:
        assert np.array_equal(fam0[key], fam1[key]), key


def test_argument_and_state_errors(capi):
    pb = BR.problem(41)
    pr = BR.params(pb)
    ctx = capi.Context(pb)
    try:
        for D in (-1, 41, 1 << 20):
            with pytest.raises(capi.CafeError, match="code 1: cafe_branch_change: max_change"):
                ctx.branch_change(pr, max_change=D)
        for level in (0.0, 1.0, float("nan")):
            with pytest.raises(capi.CafeError, match="code 1"):
                ctx.branch_change(pr, level=level)
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.branch_change(P.Params(lambdas=np.array([-0.01]), prior=pr.prior))
        assert not ctx.branch_change(pr, max_change=40)["failed"].any()        # D = max(M, R) is the last valid one
    finally:
        ctx.close()


def test_a_missing_cell_context_is_refused_and_stays_usable(capi):
    MS = BR._tables()
    pb = MS.problem(41, "base")                              # the table with its missing cells
    assert pb.missing_counts
    pr = MS.params(pb, "base")
    ctx = capi.Context(pb)
    try:
        before, fam0 = ctx.score(pr, per_family=True)
        with pytest.raises(capi.CafeError, match=r"code 4: cafe_branch_change: the table has missing cells"):
            ctx.branch_change(pr, max_change=3)
        after, fam1 = ctx.score(pr, per_family=True)
    finally:
        ctx.close()
    assert _same(before, after) and _same(fam0["family_lnl"], fam1["family_lnl"])


# ------------------------------------------------------------------------------------------------ 5. the driver
def _read_tab(path):
    with open(path) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    return rows[0], rows[1:]


@pytest.mark.parametrize("extra,model", [(["-l", "0.004"], "Base"), (["-l", "0.004", "-k", "2", "-a", "0.7"], "Gamma")])
def test_the_driver_writes_both_reports_and_the_summary_counts_its_cells(tmp_path, extra, model):
    """synth20 with --branch-change 3 at a fixed lambda: the cells are the binding's arrays at the same parameters, and the summary's
    counts are recomputed from the cells of the per-family file."""
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    cmd = [DRIVER, "-t", os.path.join(DATA, "synth20_tree.txt"), "-i", os.path.join(DATA, "synth20_families.txt"), "--branch-change", "3", "-P", "0.1",
           "-o", str(tmp_path)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["branch_change"]["max_change"] == 3 and js["branch_change"]["failed"] == 0 and abs(js["branch_change"]["level"] - 0.9) < 1e-15
    head, rows = _read_tab(os.path.join(str(tmp_path), model + "_branch_change.tab"))
    shead, srows = _read_tab(os.path.join(str(tmp_path), model + "_branch_change_summary.tab"))
    assert head[0] == "FamilyID" and len(rows) == js["n_families"]
    assert shead[:5] == ["#Node", "mean_change", "expanded", "contracted", "clipped"] and "+-3" in shead[5]
    names = [n for n in head[1:] if any(r[1 + head[1:].index(n)] != "-" for r in rows)]          # every node but the root
    assert len(names) == len(head) - 2 and [r[0] for r in srows] == names
    clipped_total = 0
    for row in srows:
        col = head.index(row[0])
        mean_sum, up, down, clipped = 0.0, 0, 0, 0
        for r in rows:
            mean, mode, iv, below, above = r[col].split(":")
            lo, hi = (int(x) for x in iv.strip("[]").split(","))
            assert -4 <= lo <= hi <= 4 and -3 <= int(mode) <= 3 and 0.0 <= float(below) <= 1.0 and 0.0 <= float(above) <= 1.0
            mean_sum += float(mean)
            up += lo > 0
            down += hi < 0
            clipped += lo < -3 or hi > 3
        assert (int(row[2]), int(row[3]), int(row[4])) == (up, down, clipped), row
        assert abs(float(row[1]) - mean_sum) <= 1e-5 * max(1.0, sum(abs(float(r[col].split(":")[0])) for r in rows)), row     # cells print 6 digits
        clipped_total += clipped
    assert js["branch_change"]["clipped"] == clipped_total

    from cafexp_amd import capi
    species, ids, counts = table("synth20_families.txt")
    pb = P.build_problem(P.parse_newick(read("synth20_tree.txt")), species, ids, counts)
    assert pb.n_families == js["n_families"]
    pr = P.Params(lambdas=np.array(js["lambda"]), prior=P.prior_uniform(pb.max_root_family_size))
    K = 1
    if model == "Gamma":
        K = 2
        pr.multipliers, pr.cat_probs = np.array(js["multipliers"]), np.full(2, 0.5)
    ctx = capi.Context(pb, max_categories=K)
    try:
        got = ctx.branch_change(pr, max_change=3, level=0.9, pmf=False, alpha=js.get("alpha", 1.0))
    finally:
        ctx.close()
    assert [r[0] for r in rows] == list(pb.family_ids)
    ch, order, q = MR.children_of(pb), [], [MR.root_of(pb)]  # the driver's columns: reverse level order, as <Model>_count.tab
    while q:
        v = q.pop(0)
        order.append(v)
        q.extend(ch[v])
    order = order[::-1]
    assert len(order) == len(head) - 1
    for col, v in enumerate(order):
        for f in range(pb.n_families):
            cell = rows[f][1 + col]
            if v == MR.root_of(pb):
                assert cell == "-"
                continue
            want = "%.6g:%d:[%d,%d]:%.6g:%.6g" % (got["mean"][f, v], got["mode"][f, v], got["lo"][f, v], got["hi"][f, v], got["below"][f, v], got["above"][f, v])
            assert cell == want, (f, v, cell, want)
