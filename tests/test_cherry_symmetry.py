"""A cherry whose two leaves use the same matrix (equal quantized branch length, same lambda index) keeps ONE panel column for
the leaf counts (a, b) and (b, a): the column is P[s][a] * P[s][b], each factor formed from its leaf's count alone, and an
IEEE product does not depend on the order of its factors (cafe_schedule.hip, plan_patterns).  Checked here:
  * the columns merge where the rule says and nowhere else -- column counts of the library (cafe_debug_column_extents)
    against a restatement in numpy, children first;
  * no result bit changes: default against CAFE_NO_CHERRY_SWAP=1 (ordered pairs everywhere) and against one column per
    family at every node (subtree_dedup=False), call for call with changing parameters.
There are no tolerances: every comparison is on the bits."""
import numpy as np
import pytest

from cafexp_amd import problem as P, synth
from cafexp_amd.gamma_rates import discrete_gamma

pytestmark = pytest.mark.gpu

T4 = "((A:1,B:1):1,(C:1,D:2):2);"                          # (A, B) symmetric; (C, D): unequal branch lengths
T6 = "((((A:1,B:1):1,C:2):1,D:3):1,(E:1,F:2):4);"           # a symmetric cherry with a non-root parent and grandparent
T_POLY = "((A:1,B:1,C:1):1,(D:1,E:2):2);"                   # two equal-length leaves AND a third child (a leaf)
T_SIB = "((A:1,B:1,(C:1,D:2):1):1,(E:1,F:2):2);"            # two equal-length leaves plus an interior sibling
# largest count drawn per leaf (uniform on 0..hi): A, B wide enough that ordered and unordered pairs pad to different
# multiples of 128 columns, the others narrow enough that every node has at most half its parent's patterns (below)
HI4 = dict(A=12, B=12, C=12, D=12)
HI6 = dict(A=12, B=12, C=3, D=2, E=2, F=2)
HI_POLY = dict(A=12, B=12, C=3, D=3, E=3)
HI_SIB = dict(A=12, B=12, C=1, D=1, E=3, F=3)


@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


def _problem(newick, hi, n_families, M, seed, lambda_newick=None, n_deviations=0):
    rng = np.random.default_rng(seed)
    species = sorted(hi)
    counts = np.stack([rng.integers(0, hi[s] + 1, size=n_families) for s in species], axis=1).astype(np.int32)
    counts[0] = [min(1, hi[s]) for s in species]
    counts[1] = [min(2, hi[s]) if s == "A" else min(1, hi[s]) for s in species]     # (2, 1) and (1, 2) at (A, B) whatever the draw
    counts[2] = [min(2, hi[s]) if s == "B" else min(1, hi[s]) for s in species]
    lam_tree = P.parse_newick(lambda_newick, lambda_tree=True) if lambda_newick else None
    return P.build_problem(P.parse_newick(newick), species, ["f%d" % i for i in range(n_families)], counts, lambda_tree=lam_tree,
                           root_filter=False, max_family_size=M, max_root_family_size=M, n_deviations=n_deviations)


def _children(pb):
    kids = [[] for _ in range(pb.n_nodes)]
    for v in range(pb.n_nodes):
        if pb.parent[v] >= 0:
            kids[pb.parent[v]].append(v)
    return kids


def _symmetric_cherry(pb, inner, leaves):
    """The rule: exactly two children, both leaves, on the same matrix (time quantized like quantize_time, same lambda index)."""
    if inner or len(leaves) != 2:
        return False
    a, b = leaves
    return int(pb.branch_length[a] * 1000) == int(pb.branch_length[b] * 1000) and pb.lambda_index[a] == pb.lambda_index[b]


def _first_two_leaves(pb, inner, leaves):
    """What the rule must NOT be: the first two leaf children sorted whatever their branches and siblings."""
    return len(leaves) >= 2


def _own_patterns(pb, rule):
    """Distinct patterns of (children's pattern ids, leaf counts) per interior node, children first; the counts of the first
    two leaf children sorted where `rule` says (None: nowhere)."""
    kids, pid, own = _children(pb), {}, {}
    for v in range(pb.n_nodes):                              # post-order: children before parents
        if pb.leaf_taxon[v] >= 0:
            continue
        inner = [u for u in kids[v] if pb.leaf_taxon[u] < 0]
        leaves = [u for u in kids[v] if pb.leaf_taxon[u] >= 0]
        rows = np.stack([pid[u] for u in inner] + [pb.counts[:, pb.leaf_taxon[u]] for u in leaves], axis=1).astype(np.int64)
        if rule is not None and rule(pb, inner, leaves):
            k = len(inner)
            rows[:, k:k + 2] = np.sort(rows[:, k:k + 2], axis=1)
        _, inv = np.unique(rows, axis=0, return_inverse=True)
        pid[v] = inv.reshape(-1)
        own[v] = int(pid[v].max()) + 1
    return own


def _pad(n):
    return (n + 127) // 128 * 128


def _inner_nodes(pb):
    return [v for v in range(pb.n_nodes) if pb.leaf_taxon[v] < 0 and pb.parent[v] >= 0]


def _expected_cols(pb, rule):
    """Columns of every interior non-root node's panel: its own patterns padded to 128.  A child whose patterns are within
    15 % / 12 % of its parent's columns takes over the parent's columns instead; the tables here keep
    every node at no more than half its parent's patterns, so that rule is never in play."""
    own = _own_patterns(pb, rule)
    for v in _inner_nodes(pb):
        assert 2 * own[v] <= own[pb.parent[v]], (pb.node_names[v], own[v], own[pb.parent[v]])
    return {pb.node_names[v]: _pad(own[v]) for v in _inner_nodes(pb)}


def _library_cols(ctx, pb):
    return {pb.node_names[v]: len(ctx.column_extents(v, 0)) for v in _inner_nodes(pb)}


def _context(capi, monkeypatch, pb, K=1, swap=True, **kw):
    if swap:
        monkeypatch.delenv("CAFE_NO_CHERRY_SWAP", raising=False)
    else:
        monkeypatch.setenv("CAFE_NO_CHERRY_SWAP", "1")
    ctx = capi.Context(pb, max_categories=K, **kw)
    monkeypatch.delenv("CAFE_NO_CHERRY_SWAP", raising=False)
    return ctx


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


def _base(pb, lam):
    return P.Params(lambdas=np.atleast_1d(np.array(lam, dtype=np.float64)), prior=P.prior_uniform(pb.max_root_family_size))


# ------------------------------------------------------------------ merging
def test_symmetric_cherry_merges_and_an_asymmetric_one_does_not(capi, monkeypatch):
    pb = _problem(T4, HI4, 400, 260, seed=5)                 # matrix order 261: extents, hence column counts, are on
    ab, cd = pb.counts[:, pb.taxa.index("A")] * 100 + pb.counts[:, pb.taxa.index("B")], pb.counts[:, pb.taxa.index("C")] * 100 + pb.counts[:, pb.taxa.index("D")]
    ba = pb.counts[:, pb.taxa.index("B")] * 100 + pb.counts[:, pb.taxa.index("A")]
    ordered_ab, ordered_cd = len(np.unique(ab)), len(np.unique(cd))
    unordered_ab = len(np.unique(np.minimum(ab, ba)))
    assert np.intersect1d(ab[ab != ba], ba[ab != ba]).size > 0          # both (a, b) and (b, a) occur
    assert _pad(unordered_ab) < _pad(ordered_ab)                        # ... often enough to show in the padded counts
    want = _expected_cols(pb, _symmetric_cherry)
    assert want == {"AB": _pad(unordered_ab), "CD": _pad(ordered_cd)}
    ctx = _context(capi, monkeypatch, pb)
    ctx.score(_base(pb, 0.05))
    assert _library_cols(ctx, pb) == want
    ctx.close()
    ctx = _context(capi, monkeypatch, pb, swap=False)
    ctx.score(_base(pb, 0.05))
    assert _library_cols(ctx, pb) == {"AB": _pad(ordered_ab), "CD": _pad(ordered_cd)} == _expected_cols(pb, None)
    ctx.close()


def test_merged_columns_propagate_to_parent_and_grandparent(capi, monkeypatch):
    pb = _problem(T6, HI6, 6000, 260, seed=6)
    want, ordered = _expected_cols(pb, _symmetric_cherry), _expected_cols(pb, None)
    for name in ("AB", "ABC", "ABCD"):                       # the cherry, its parent, its grandparent: all shrink
        assert want[name] < ordered[name], (name, want, ordered)
    assert want["EF"] == ordered["EF"]
    for swap, cols in ((True, want), (False, ordered)):
        ctx = _context(capi, monkeypatch, pb, swap=swap)
        ctx.score(_base(pb, 0.05))
        assert _library_cols(ctx, pb) == cols
        ctx.close()


# ------------------------------------------------------------------ the rule's limits
@pytest.mark.parametrize("case", ["lambda", "length", "polytomy", "sibling"])
def test_nothing_merges_outside_the_rule(capi, monkeypatch, case):
    """Different lambda indices on the two leaves, unequal branch lengths, a third (leaf) child, an interior sibling: the
    product is no longer that of two factors of one matrix, (F * fa) * fb and (F * fb) * fa may differ in the last bit."""
    if case == "lambda":
        pb, node, lams = _problem(T4, HI4, 400, 260, seed=7, lambda_newick="((A:1,B:2):1,(C:1,D:1):1);"), "AB", [0.05, 0.03]
    elif case == "length":
        pb, node, lams = _problem("((A:1,B:1.5):1,(C:1,D:2):2);", HI4, 400, 260, seed=8), "AB", [0.05]
    elif case == "polytomy":
        pb, node, lams = _problem(T_POLY, HI_POLY, 3000, 260, seed=9), "ABC", [0.05]
    else:
        pb, node, lams = _problem(T_SIB, HI_SIB, 3000, 260, seed=10), "ABCD", [0.05]
    want = _expected_cols(pb, _symmetric_cherry)
    assert want == _expected_cols(pb, None)
    assert _expected_cols(pb, _first_two_leaves)[node] < want[node]      # (a rule that merged here would show in the count)
    pr = _base(pb, lams)
    got = []
    for kw in (dict(), dict(swap=False), dict(subtree_dedup=False)):
        ctx = _context(capi, monkeypatch, pb, **kw)
        got.append(ctx.score(pr, per_family=True) + (ctx.root_max(pr.lambdas),))
        if "subtree_dedup" not in kw:
            assert _library_cols(ctx, pb) == want
        ctx.close()
    for other in got[1:]:
        assert got[0][0] == other[0]
        for key in got[0][1]:
            assert _same_bits(got[0][1][key], other[1][key]), key
        assert _same_bits(got[0][2], other[2])


# ------------------------------------------------------------------ no bit changes
def _tree_problem(tree, n_dev):
    if tree == "t4":                                         # matrix order 261: zero extents, planned tile lists, row skipping
        return _problem(T4, HI4, 400, 260, seed=5, n_deviations=n_dev)
    if tree == "t4_small":                                   # matrix order 41: none of them
        return _problem(T4, HI4, 400, 40, seed=5, n_deviations=n_dev)
    if tree == "t6":
        return _problem(T6, HI6, 6000, 260, seed=6, n_deviations=n_dev)
    if tree == "yule_289":                                   # a simulated table on an ultrametric tree, largest count 230: order 289
        return synth.make_problem(n_taxa=12, n_families=400, max_count=230, lam_sim=0.003, seed=17, root_cap=115, n_deviations=n_dev)[0]
    return synth.make_problem(n_taxa=12, n_families=300, max_count=60, lam_sim=0.004, seed=3, root_cap=40, n_deviations=n_dev)[0]   # largest count 60: order below 256


@pytest.mark.parametrize("model", ["base", "gamma3", "err3", "err5", "two_rate"])
@pytest.mark.parametrize("tree", ["t4", "t4_small", "t6", "yule_289", "yule_small"])
def test_no_result_bit_changes(capi, monkeypatch, tree, model):
    """-lnL, every per-family array and root_max of the default context against ordered pairs (CAFE_NO_CHERRY_SWAP=1) and one
    column per family (subtree_dedup=False), over three calls on the same contexts: the second with other rates (other
    matrices, other extents), the third with the first's again."""
    n_dev = {"err3": 3, "err5": 5}.get(model, 0)
    pb = _tree_problem(tree, n_dev)
    assert (pb.matrix_size >= 256) == (tree in ("t4", "t6", "yule_289"))
    kids = _children(pb)
    n_sym = sum(_symmetric_cherry(pb, [u for u in kids[v] if pb.leaf_taxon[u] < 0], [u for u in kids[v] if pb.leaf_taxon[u] >= 0])
                for v in range(pb.n_nodes) if pb.leaf_taxon[v] < 0)
    assert n_sym >= 1
    hand = tree in ("t4", "t4_small", "t6")
    lam = 0.05 if hand else 0.004
    K = 3 if model == "gamma3" else 1
    em = None
    if n_dev == 3:
        em = P.error_model_table(P.default_error_model(pb.max_family_size)[:1] + [[0.05, 0.9, 0.05]], pb.max_family_size)
    if n_dev == 5:
        em = P.error_model_table([[0.0, 0.0, 0.8, 0.15, 0.05], [0.0, 0.1, 0.75, 0.1, 0.05], [0.05, 0.1, 0.7, 0.1, 0.05]], pb.max_family_size)
    probs, mult = discrete_gamma(3, 0.9) if K == 3 else (None, None)
    prior = P.prior_uniform(pb.max_root_family_size)
    prs = [P.Params(lambdas=np.array([l]), prior=prior, multipliers=mult, cat_probs=probs, error_model=em) for l in (lam, lam * 0.3, lam)]
    got, flops = [], []
    for kw in (dict(), dict(swap=False), dict(subtree_dedup=False)):
        ctx = _context(capi, monkeypatch, pb, K=K, **kw)
        if model == "two_rate":
            ctx.set_death_rates([lam * 1.5])
        calls = []
        for pr in prs:
            calls.append(ctx.score(pr, alpha=0.9, per_family=True) + (ctx.root_max(pr.lambdas),))
        got.append(calls)
        flops.append(ctx.stats()["gemm_flops"])
        ctx.close()
    for call in got[0]:                                     # (equal bits of finite values, not of NaNs or infinities)
        assert np.isfinite(call[0]) and np.isfinite(call[1]["family_lnl"]).all() and not call[1]["failed"].any()
    if hand:
        assert flops[0] < flops[1]                         # fewer GEMM columns: the merge is live in what is compared
    else:
        assert flops[0] <= flops[1]
    for other in got[1:]:
        for mine, theirs in zip(got[0], other):
            assert np.float64(mine[0]).view(np.uint64) == np.float64(theirs[0]).view(np.uint64)
            assert set(mine[1]) == set(theirs[1])
            for key in mine[1]:
                assert _same_bits(mine[1][key], theirs[1][key]), key
            assert _same_bits(mine[2], theirs[2])
    # (the third call repeats the first: a context carries nothing from call to call)
    assert got[0][0][0] == got[0][2][0] or (np.isnan(got[0][0][0]) and np.isnan(got[0][2][0]))
