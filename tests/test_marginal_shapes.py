"""cafe_marginal_reconstruct (csrc/marginal.hip) away from the three geometries of test_marginal_gpu.py: every guard of the
fp64 GEMM's 64-row tile, 16-deep K step and diagonal mask, the root range either side of M by more than a row tile, row 0
of P (which is not stored), store against multiply in the up pass, products of more than kMaxProd = 6 factors, the last
partial column batch, gamma x error model, and batches that mix failed and good families.

Reference and tolerance are test_marginal_gpu's: marginal_ref.updown fed the matrices the call itself built
(MR.context_matrices); doubles |d| <= 1e-12 + 1e-10 |ref|, integers exact except where the reference itself is within
1e-9 of a tie (under 1 % of a case's cells), failed exactly (_compare).  Every family meant to succeed has reference
Z >= 1e-250, asserted, so that no comparison rests on denormal sums.

The CPU tests say what the GPU tests can see: the extents reach every guard (arithmetic on PAIRS), the inputs put
posterior weight on the K tail, the last row tile and row 0 (asserted on the reference, 1e-6 of Z: four orders above the
tolerance), and six deliberately wrong passes are each told from the right one at every pair of order <= 513."""
import dataclasses
import functools

import numpy as np
import pytest

import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import _explicit_problem
from oracle import oracle as O
from test_gpu_parity import _random_problem
from test_marginal_gpu import _compare, _invariants
from test_per_family_shapes import FIVE_TAPS, THREE_TAPS

kMT, kKT, kBN, kMaxProd = 64, 16, 128, 6                     # marginal.hip's row tile, K step, column tile, factors per product launch

# (M, R).  Up pass: nr in {M, R} rows (R under the root), nk = M + 1.  Down and split passes: nr = M + 1, nk in {M, R}.
PAIRS = [(2, 2), (15, 14), (40, 30), (63, 64), (64, 63), (65, 129), (126, 62), (128, 128), (191, 100), (60, 200), (257, 385),
         (320, 255), (383, 512), (512, 448), (750, 640), (600, 750), (1025, 1100), (1278, 1150), (2047, 1983), (1920, 2047)]
CPU_PAIRS = [p for p in PAIRS if max(p) + 1 <= 513]          # the reference alone, with oracle matrices

SWEEP_TREE = "(((A:3,B:5):4,(C:2,D:6):3):5,(E:4,(F:1,G:2):2):3,H:7);"
# The rule: one lambda at every order.  0.1 keeps the longest branch (7) below saturation (lambda t < 1) and is large
# enough that a root held to R < M still reaches leaves at M, and that a clade of zeros is plausible, at every pair.
SWEEP_LAMBDA = 0.1
Z_MIN = 1e-250


def sweep_prior(R):
    """prior[s - 1] ~ 1 / s: not uniform, so that reading it one place off changes every weight."""
    w = 1.0 / np.arange(1, R + 1)
    return (w / w.sum()).astype(np.float32)


def sweep_rows(M):
    """Families scaled to M: small counts; every leaf at M; a mix of M - 1 and M; counts near M / 4; counts near 3 M / 4;
    the deep clade ((A,B),(C,D)) at 0 with the other leaves positive; all zeros but one leaf."""
    q, h, one = max(1, M // 4), max(1, 3 * M // 4), max(1, M // 16)
    rows = [dict(A=3, B=5, C=2, D=4, E=1, F=2, G=3, H=2),
            dict.fromkeys("ABCDEFGH", M),
            dict(A=M, B=M - 1, C=M, D=M - 1, E=M - 1, F=M, G=M, H=M - 1),
            dict(A=q, B=q - q // 12, C=q + q // 16, D=q, E=q + 1, F=q - q // 8, G=q + q // 10, H=q),
            dict(A=h, B=h - h // 12, C=h + h // 16, D=h, E=h + 1, F=h - h // 8, G=h + h // 10, H=h),
            dict(A=0, B=0, C=0, D=0, E=2, F=1, G=1, H=2),
            dict(A=one, B=0, C=0, D=0, E=0, F=0, G=0, H=0)]
    return [{s: int(min(max(c, 0), M)) for s, c in r.items()} for r in rows]


def sweep_case(M, R):
    pb = _explicit_problem(SWEEP_TREE, sweep_rows(M), M, R)
    assert pb.matrix_size == max(M, R) + 1 and pb.max_family_size == M and pb.max_root_family_size == R
    return pb, P.Params(lambdas=np.array([SWEEP_LAMBDA]), prior=sweep_prior(R))


def _levels(pb):
    return (0.95, 0.5) if pb.matrix_size <= 513 else (0.95,)


def _interior(pb):
    return [v for v in range(pb.n_nodes) if pb.leaf_taxon[v] < 0]


def _assert_no_underflow(ref, good=None):
    z = ref["Z"] if good is None else ref["Z"][good]
    assert np.all(z >= Z_MIN), z.min()


def _assert_weight_on_the_guards(pb, ref):
    """On the reference (un-normalised posteriors and G[0] from updown(detail=True)): the inputs put at least 1e-6 of Z
    where the kernel's guards are."""
    M, root, ch = pb.max_family_size, MR.root_of(pb), MR.children_of(pb)
    inner = [v for v in _interior(pb) if v != root]
    post = ref["post"][:, inner, :M + 1] / ref["Z"][:, None, None]
    k_tail = float(post[:, :, kKT * (M // kKT):].sum(axis=2).max())
    row_tail = float(post[:, :, kMT * (M // kMT):].sum(axis=2).max())
    below = [v for p in inner for v in ch[p] if pb.leaf_taxon[v] < 0]        # interior children of non-root interior nodes
    g = ref["row0"][:, below, :]
    row0 = float((g[:, :, 0] / g[:, :, 1]).max())
    print("M %d R %d: weight on the last K step %.3g, the last row tile %.3g, row 0 of G %.3g" % (M, pb.max_root_family_size, k_tail, row_tail, row0))
    assert k_tail >= 1e-6 and row_tail >= 1e-6 and row0 >= 1e-6
    return k_tail, row_tail, row0


# ---------------------------------------------------------------------------------------------------- CPU
def test_the_pairs_reach_every_guard():
    assert 18 <= len(PAIRS) <= 24 and len(set(PAIRS)) == len(PAIRS)
    want64, want16 = {0, 1, 63}, {0, 1, 15}
    assert want64 <= {M % kMT for M, R in PAIRS}             # up pass, nr = M
    assert want64 <= {R % kMT for M, R in PAIRS}             # up pass under the root, nr = R
    assert want64 <= {(M + 1) % kMT for M, R in PAIRS}       # down and split passes, nr = M + 1
    assert want16 <= {(M + 1) % kKT for M, R in PAIRS}       # up pass, nk = M + 1
    assert want16 <= {M % kKT for M, R in PAIRS}             # down and split passes, nk = M
    assert want16 <= {R % kKT for M, R in PAIRS}             # down and split passes under the root, nk = R
    assert any(max(M, R) + 1 <= kKT for M, R in PAIRS)       # fewer sizes than one K step
    assert any(kKT < M + 1 < kMT for M, R in PAIRS)          # more than one K step, less than one row tile
    assert any(M == R for M, R in PAIRS)
    assert any(R <= M - kMT for M, R in PAIRS)               # whole row tiles of the i > j split start at kbeg = r0 >= nk
    assert any(M + 1 > kMT and R <= kMT * (M // kMT) for M, R in PAIRS)      # ... and at least one such tile really exists
    assert any(R >= M + kMT for M, R in PAIRS)               # kend = min(nk, r0 + 63) cuts; more row tiles than K data under the root
    orders = [max(M, R) + 1 for M, R in PAIRS]
    assert 751 in orders and 2048 in orders and max(orders) == 2048
    at_limit = [(M, R) for M, R in PAIRS if max(M, R) + 1 == 2048]
    assert any(M > R for M, R in at_limit) and any(R > M for M, R in at_limit)
    for M, R in PAIRS:
        assert all(0 <= c <= M for r in sweep_rows(M) for c in r.values())
    assert all(max(p) + 1 <= 513 for p in CPU_PAIRS) and (383, 512) in CPU_PAIRS and len(CPU_PAIRS) >= 12


def test_the_sweep_tree_has_every_kind_of_node():
    pb, _ = sweep_case(40, 30)
    ch, root = MR.children_of(pb), MR.root_of(pb)
    leaf = lambda v: pb.leaf_taxon[v] >= 0
    inner = _interior(pb)
    assert any(all(not leaf(c) for c in ch[v]) for v in inner)                                   # (a) store, then multiply
    assert any(any(leaf(c) for c in ch[v]) and any(not leaf(c) for c in ch[v]) for v in inner)    # (b) product, then multiply
    assert any(leaf(c) for c in ch[root])                                                         # (c)
    depth = lambda v: 0 if v == root else 1 + depth(int(pb.parent[v]))
    assert max(depth(v) for v in range(pb.n_nodes)) >= 3                                          # (d)
    assert any(len(ch[v]) == 3 for v in inner)                                                    # (e)
    # a non-root interior node with an interior child: where the row-0 term of the down epilogue can carry weight
    assert any(v != root and any(not leaf(c) for c in ch[v]) for v in inner)


@functools.lru_cache(maxsize=None)
def _cpu_case(M, R):
    pb, pr = sweep_case(M, R)
    mats = MR.oracle_matrices(pb, pr, O)
    return pb, pr, mats, MR.updown(pb, pr, mats, 0.95, detail=True)


@pytest.mark.parametrize("M,R", CPU_PAIRS)
def test_the_reference_alone_has_few_ties_no_underflow_and_weight_on_the_guards(M, R):
    pb, pr, mats, ref = _cpu_case(M, R)
    assert not ref["failed"].any()
    _assert_no_underflow(ref)
    _assert_weight_on_the_guards(pb, ref)
    for level in _levels(pb):
        r = ref if level == 0.95 else MR.updown(pb, pr, mats, level)
        share = _compare(r, r, "reference alone M %d R %d level %.2f" % (M, R, level))          # asserts the share < 1 %
        assert share < 0.01


def _edited(mats, edit):
    out = []
    for row in mats:
        new = []
        for m in row:
            new.append(None if m is None else m.copy())
            if m is not None:
                edit(new[-1])
        out.append(new)
    return out


def _drop_k_tail(M):
    def edit(m):
        m[:, kKT * ((M + 1) // kKT):] = 0.0                  # the up pass's last, partial K step: child sizes j
    return edit


def _drop_last_row_tile(M):
    def edit(m):
        m[1 + kMT * ((M - 1) // kMT):, :] = 0.0              # the up pass's last row tile at nr = M: parent sizes i = r + 1
    return edit


def _drop_row0(m):
    m[0, 0] = 0.0                                            # P[0][j] = delta(j, 0): the term both epilogues add


MATRIX_MUTANTS = {"k_tail_dropped": _drop_k_tail, "last_row_tile_dropped": _drop_last_row_tile, "row0_term_dropped": lambda M: _drop_row0}
# Pairs where a mutant changes nothing by construction.  The K tail is empty where 16 divides M + 1.  Where R >= M + 64 no
# count exceeds M, so a root of size R would have to shrink by 64 or more on all three of its branches: its posterior
# weight there is below 1e-25 of Z (asserted; measured below 1e-30), far under one ulp, and a pass that stops at R - 1
# computes the same doubles.
NO_OP = {"k_tail_dropped": {(M, R) for M, R in CPU_PAIRS if (M + 1) % kKT == 0},
         "root_range_stops_short": {(M, R) for M, R in CPU_PAIRS if R >= M + kMT}}


def _told_apart(mut, ref, label):
    """True if _compare(mut, ref) raises AND the difference is not marginal: failed or NaN patterns differ, an integer
    differs away from a tie, or a double is off by more than 100 x the bound."""
    big = False
    for key in ("mean", "p_increase", "p_decrease", "log_evidence"):
        g, r = np.asarray(mut[key]), np.asarray(ref[key])
        if not np.array_equal(np.isnan(g), np.isnan(r)):
            big = True
            continue
        ok = ~np.isnan(r)
        if ok.any() and np.max(np.abs(g[ok] - r[ok]) / (1e-12 + 1e-10 * np.abs(r[ok]))) > 100:
            big = True
    big = big or not np.array_equal(mut["failed"], ref["failed"])
    for key, mask in zip(("mode", "lo", "hi"), MR.excused(ref)):
        big = big or bool(np.any((np.asarray(mut[key]) != np.asarray(ref[key])) & ~mask))
    if not big:
        return False
    with pytest.raises(AssertionError):
        _compare(mut, ref, label)
    return True


@pytest.mark.parametrize("M,R", CPU_PAIRS)
def test_the_inputs_tell_a_wrong_pass_from_a_right_one(M, R):
    """Six mutants of the reference -- three by editing the matrices handed to updown, three through its `mutant` hook --
    against the right pass on the sweep's own inputs, oracle.build_matrix matrices.  Each is caught at every pair outside
    NO_OP."""
    pb, pr, mats, ref = _cpu_case(M, R)
    root = MR.root_of(pb)
    for name in list(MATRIX_MUTANTS) + list(MR.MUTANTS):
        if name in MATRIX_MUTANTS:
            mut = MR.updown(pb, pr, _edited(mats, MATRIX_MUTANTS[name](M)), 0.95)
        else:
            mut = MR.updown(pb, pr, mats, 0.95, mutant=name)
        label = "%s M %d R %d" % (name, M, R)
        if (M, R) in NO_OP.get(name, ()):
            if name == "root_range_stops_short":
                assert np.all(ref["post"][:, root, R] <= 1e-25 * ref["Z"]), label
            for key in ("mean", "p_increase", "p_decrease", "log_evidence", "mode", "lo", "hi", "failed"):
                assert np.array_equal(mut[key], ref[key], equal_nan=True), (label, key)
            print("%s: changes nothing here by construction" % label)
            continue
        assert _told_apart(mut, ref, label), label
        print("%s: caught" % label)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _K(pr):
    return 1 if pr.multipliers is None else len(pr.multipliers)


def _interval_invariants(got, ref):
    """test_marginal_gpu._invariants wherever it is one.  lo <= mode <= hi is no property of a posterior that is cut off
    at M or R: where it rises to the cut and the last size holds less than (1 - level) / 2 of the mass (every leaf at M
    under a root held to R < M, level 0.5), the mode is the last size and hi lies below it.  The sweep makes such
    posteriors on purpose, so: the mode may leave the interval exactly where the reference's does, lo <= hi always, and
    _invariants itself on the rows where the reference keeps its mode inside."""
    ok = got["failed"] == 0
    assert np.all(got["lo"][ok] <= got["hi"][ok])
    out = lambda r: ((r["mode"] < r["lo"]) | (r["mode"] > r["hi"]))[ok]
    assert np.array_equal(out(got), out(ref))
    rows = np.where(ok)[0][~out(ref).any(axis=1)]
    _invariants({k: v[rows] for k, v in got.items()})
    s = (got["p_increase"] + got["p_decrease"])[ok]
    s = s[~np.isnan(s)]
    assert np.all(s >= 0) and np.all(s <= 1 + 1e-12)


def _run(capi, pb, pr, label, alpha=1.0, levels=None, good=None, **ctx_args):
    """One context, one call per level, compared with the reference on the matrices the call built.  Returns the last
    level's (got, ref); ref carries updown's detail."""
    K = _K(pr)
    ctx = capi.Context(pb, max_categories=K, **ctx_args)
    try:
        mats = None
        for level in levels or _levels(pb):
            got = ctx.marginal_reconstruct(pr, level=level, alpha=alpha)
            if mats is None:
                mats = MR.context_matrices(ctx, pb, K)
            ref = MR.updown(pb, pr, mats, level, detail=True)
            _assert_no_underflow(ref, good)
            _compare(got, ref, "%s level %.2f" % (label, level))
            _interval_invariants(got, ref)
    finally:
        ctx.close()
    ok = got["failed"] == 0
    root = MR.root_of(pb)
    assert np.all(np.isnan(got["p_increase"][:, root])) and np.all(np.isnan(got["p_decrease"][:, root]))
    if pr.error_model is None:
        leaves = np.where(pb.leaf_taxon >= 0)[0]
        for key in ("mode", "lo", "hi", "mean"):
            assert np.array_equal(got[key][ok][:, leaves], pb.counts[ok][:, pb.leaf_taxon[leaves]]), key
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("M,R", PAIRS)
def test_sweep_of_the_gemm_extents(capi, M, R):
    """2. One problem per pair on SWEEP_TREE, families scaled to M, lambda 0.1 at every order."""
    pb, pr = sweep_case(M, R)
    got, ref = _run(capi, pb, pr, "sweep M %d R %d" % (M, R))
    assert not got["failed"].any()
    _assert_weight_on_the_guards(pb, ref)


STAR8 = "(A:1,B:2,C:1.5,D:3,E:0.5,F:2.5,G:1,H:2);"
SEVEN_LEAVES_TWO_CLADES = "((A:1,B:1,C:2,D:0.5,E:1,F:3,G:2,(H:1,I:2):1,(J:2,K:1):0.5):2,L:4);"
SEVEN_LEAVES_TWO_CLADES_LAMBDAS = "((A:1,B:1,C:2,D:2,E:1,F:1,G:2,(H:1,I:2):2,(J:2,K:1):1):1,L:2);"
EIGHT_CLADES = "(((A:1,B:2):1,(C:1,D:1):2,(E:2,F:1):1,(G:1,H:3):1,(I:1,J:1):2,(K:2,L:2):1,(M:1,N:1):1.5,(O:3,P:1):0.5):2,Q:4);"
TREES = {
    "star_of_8_leaves": (STAR8, None),
    "7_leaves_and_2_clades": (SEVEN_LEAVES_TWO_CLADES, SEVEN_LEAVES_TWO_CLADES_LAMBDAS),
    "8_clades": (EIGHT_CLADES, None),
    "caterpillar": ("((((A:1,B:1):1,C:2):1,D:3):1,E:4);", None),
    "balanced": ("(((A:1,B:1):1,(C:1,D:1):1):1,((E:1,F:1):1,(G:1,H:1):1):1);", None),
}
TREE_ORDERS = [(40, 30), (250, 299)]                         # orders 41 and 300, as test_per_family_shapes.test_tree_shapes


def _tree_problem(name, M, R):
    newick, lambda_newick = TREES[name]
    pb = _random_problem(np.random.default_rng(5 + sorted(TREES).index(name)), newick, 70, M, R, 12)
    lambdas = np.array([0.02])
    if lambda_newick:
        index = {nd.key(): nd.lambda_index - 1 for nd in P.parse_newick(lambda_newick, lambda_tree=True).postorder()}
        pb = dataclasses.replace(pb, lambda_index=np.array([index[k] for k in pb.node_names], dtype=np.int32), n_lambdas=2, single_lambda=False)
        assert set(pb.lambda_index) == {0, 1}
        lambdas = np.array([0.02, 0.006])
    return pb, P.Params(lambdas=lambdas, prior=P.prior_uniform(R))


def test_the_trees_pass_the_product_limit():
    """CPU: what the three wide trees are for."""
    def widest(name):
        pb, _ = _tree_problem(name, 40, 30)
        ch = MR.children_of(pb)
        leaves = max(sum(1 for c in ch[v] if pb.leaf_taxon[c] >= 0) for v in range(pb.n_nodes))
        clades = max(sum(1 for c in ch[v] if pb.leaf_taxon[c] < 0) for v in range(pb.n_nodes))
        return leaves, clades, pb.n_lambdas
    assert widest("star_of_8_leaves") == (8, 0, 1)           # up product of 8 leaves; down product over 7 leaf siblings
    assert widest("7_leaves_and_2_clades") == (7, 2, 2)      # up product of 7 leaves, then two multiplies; two lambdas
    assert widest("8_clades") == (2, 8, 1)                   # store, seven multiplies; down product over 7 sibling panels
    assert min(8 - 1, 7) > kMaxProd


@pytest.mark.gpu
@pytest.mark.parametrize("M,R", TREE_ORDERS)
@pytest.mark.parametrize("name", sorted(TREES))
def test_trees_and_products(capi, name, M, R):
    """4. Nodes of seven and more children (product() chains launches past six factors), and test_gpu_parity's shapes."""
    pb, pr = _tree_problem(name, M, R)
    got, _ = _run(capi, pb, pr, "%s M %d R %d" % (name, M, R))
    assert not got["failed"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("M,R", TREE_ORDERS)
def test_a_batch_of_failed_and_good_families(capi, M, R):
    """4. A's branch quantizes to t_q = 0: its matrix is e_0 in row 0 and zero below, so a family is possible only with
    A = 0 under an extinct parent, hence B = 0 too.  Half the families are made so; the others fail, in the same batch."""
    pb = _random_problem(np.random.default_rng(5), "((A:0.0004,B:1):1,C:2);", 70, M, R, 12)
    counts = pb.counts.copy()
    a, b = pb.taxa.index("A"), pb.taxa.index("B")
    counts[::2, [a, b]] = 0
    pb = dataclasses.replace(pb, counts=counts)
    possible = (counts[:, a] == 0) & (counts[:, b] == 0)
    assert possible.sum() >= 20 and (~possible).sum() >= 20
    pr = P.Params(lambdas=np.array([0.02]), prior=P.prior_uniform(R))
    got, ref = _run(capi, pb, pr, "t_q = 0 M %d R %d" % (M, R), good=possible)
    assert np.array_equal(got["failed"] == 0, possible) and np.array_equal(ref["failed"] == 0, possible)
    for key in ("mean", "p_increase", "p_decrease"):
        assert np.all(np.isnan(got[key][~possible])), key
    assert np.all(np.isnan(got["log_evidence"][~possible])) and np.all(np.isfinite(got["log_evidence"][possible]))
    for key in ("mode", "lo", "hi"):
        assert np.all(got[key][~possible] == -1) and np.all(got[key][possible] >= 0), key
    ab = int(pb.parent[int(np.where(pb.leaf_taxon == a)[0][0])])
    assert np.all(got["mode"][possible, ab] == 0) and np.all(got["hi"][possible, ab] == 0)      # the parent of A is extinct
    assert np.all(got["p_decrease"][possible, ab] >= 1 - 1e-12) and np.all(got["p_increase"][possible, ab] == 0.0)


TAP_TREE = "((A:3,B:5,C:2,(D:4,E:6):3):4,(F:6,G:1):2);"


def _tap_problem(taps, M, R, n_fam=64, seed=None):
    """The tree and the count rows of test_per_family_shapes.test_error_model_taps_at_the_ends_of_the_range."""
    tree = P.parse_newick(TAP_TREE)
    species = ["A", "B", "C", "D", "E", "F", "G"]
    counts = np.random.default_rng(11 + taps + M if seed is None else seed).integers(0, 15, size=(n_fam, 7)).astype(np.int32)
    counts[0] = 0
    counts[1] = [1, 0, 2, 0, 1, 0, 3]
    counts[2] = [0, 1, 1, 0, 0, 1, 0]
    counts[3] = M
    counts[4] = [M, M - 1, M, M - 1, M - 2, M, M - 1]
    counts[5] = M - 1
    counts[6] = [M - 3, M - 1, M, M - 2, M, M - 1, M - 4]
    pb = P.build_problem(tree, species, ["f%d" % i for i in range(n_fam)], counts, root_filter=False, n_deviations=taps,
                         max_family_size=M, max_root_family_size=R)
    for c in (0, 1, M - 1, M):
        assert (pb.counts == c).any(), c
    em = P.error_model_table(FIVE_TAPS if taps == 5 else THREE_TAPS, M)
    assert em.shape == (M + 1, taps) and em[M, -1] > 0       # the tap that falls above M carries weight
    return pb, em


@pytest.mark.gpu
@pytest.mark.parametrize("M,R", [(40, 30), (140, 150)])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("taps", [3, 5])
def test_gamma_times_error_model_with_taps_at_the_ends(capi, taps, K, M, R):
    """5. Counts 0, 1, M - 1 and M at leaves under 3-tap and 5-tap tables, base and gamma K = 3: the only cases where the
    leaf summary kernel does more than copy the count."""
    pb, em = _tap_problem(taps, M, R)
    pr = P.Params(lambdas=np.array([0.02]), prior=P.prior_uniform(R), error_model=em)
    alpha = 1.0
    if K == 3:
        alpha = 0.5
        pr.cat_probs, pr.multipliers = O.discrete_gamma(3, alpha)
    got, ref = _run(capi, pb, pr, "taps %d K %d M %d R %d" % (taps, K, M, R), alpha=alpha, levels=(0.95, 0.5))
    assert not got["failed"].any()
    leaves = np.where(pb.leaf_taxon >= 0)[0]
    counts = pb.counts[:, pb.leaf_taxon[leaves]]
    assert np.any(ref["lo"][:, leaves] < ref["hi"][:, leaves]) and np.any(ref["mode"][:, leaves] != counts)    # more than a copy
    for key, mask in zip(("mode", "lo", "hi"), MR.excused(ref)):
        assert np.array_equal(got[key][:, leaves][~mask[:, leaves]], ref[key][:, leaves][~mask[:, leaves]]), key
    d = np.abs(got["mean"][:, leaves] - ref["mean"][:, leaves])
    assert np.all(d <= 1e-12 + 1e-10 * np.abs(ref["mean"][:, leaves]))
    assert np.all(np.abs(got["mean"][:, leaves] - counts) <= taps // 2)


@pytest.mark.gpu
def test_three_column_tiles_of_distinct_families(capi):
    """6. 300 distinct families at order 130 (three row tiles down, the last of two rows; three column tiles, no
    duplicates), every family against the reference."""
    pb = _random_problem(np.random.default_rng(61), SWEEP_TREE, 300, 129, 100, 12)
    assert len(np.unique(pb.counts, axis=0)) == 300 and pb.matrix_size == 130
    pr = P.Params(lambdas=np.array([0.02]), prior=P.prior_uniform(100))
    got, _ = _run(capi, pb, pr, "300 distinct families", levels=(0.95,))
    assert not got["failed"].any()


def _per_col(pb, n_tap):
    """marginal_impl's own workspace formula: bytes per column."""
    n, nI = pb.n_nodes, len(_interior(pb))
    nL, rows = n - nI, pb.matrix_size
    doubles = 4 * nI * rows + 2 * rows + nL * (n_tap + 2) + 2 * nI + 1 + 3 * n
    return doubles * 8 + 3 * n * 4


@pytest.mark.gpu
def test_a_partial_last_batch_changes_no_bit(capi):
    """6. K = 3 with a 3-tap error model, 300 distinct families (384 padded columns): one batch, batches of 256 + 128 (the
    last one has ld = 128 < cols = 256, while the leaf, branch and summary arrays keep stride cols) and three batches of
    128 give the same bits in every output; the one-batch run is compared with the reference.  The context exposes
    nothing that shows the batch count: the limits come from marginal_impl's formula, cols = min(Fp, floor(limit /
    per_col) rounded down to 128)."""
    rng = np.random.default_rng(62)
    tree = P.parse_newick(SWEEP_TREE)
    names = [l.name for l in tree.leaves()]
    counts = rng.integers(0, 15, size=(300, len(names))).astype(np.int32)
    counts[0], counts[1], counts[2] = 0, 129, 128
    assert len(np.unique(counts, axis=0)) == 300
    pb = P.build_problem(tree, names, ["f%d" % i for i in range(300)], counts, root_filter=False, n_deviations=3,
                         max_family_size=129, max_root_family_size=100)
    pr = P.Params(lambdas=np.array([0.02]), prior=P.prior_uniform(100), error_model=P.error_model_table(THREE_TAPS, 129))
    pr.cat_probs, pr.multipliers = O.discrete_gamma(3, 0.5)
    per_col = _per_col(pb, 3)
    padded = -(-300 // kBN) * kBN
    assert padded == 384
    want, _ = _run(capi, pb, pr, "K 3, 3 taps, one batch", alpha=0.5, levels=(0.95,))
    assert not want["failed"].any()
    for cols in (256, 128):
        limit = cols * per_col + per_col // 2
        assert limit // per_col // kBN * kBN == cols < padded
        ctx = capi.Context(pb, max_categories=3, workspace_limit=limit)
        try:
            assert -(-ctx.stats()["n_unique_families"] // kBN) * kBN == padded
            got = ctx.marginal_reconstruct(pr, alpha=0.5)
        finally:
            ctx.close()
        for key in want:
            assert np.array_equal(got[key], want[key], equal_nan=True), (cols, key)
