"""cafe_simulate (simulate.hip, tree_sampler.h) replayed draw for draw on the host.

The device sampler is a pure function of its arguments: every draw is Philox4x32-10 keyed by the seed with counter
(family lo, family hi, node, stream).  `replay` below restates it in numpy -- the generator and uniform01 as
tree_sampler.h states them, the inverse-CDF draw as np.searchsorted(cdf_row, u * cdf_row[-1], side="left"), the
error-model step on stream 1 -- over the matrices of capi.build_matrices, cumulated over columns 0..S-1 with np.cumsum.
The GPU tests ask for EQUAL leaf_counts and node_sizes, family by family.

One difference is legitimate: the device sums a row by a 64-lane scan plus carry, numpy sequentially.  Both orders err by
at most (S - 1) * 2^-53 of the row total (2^-42 at S = 2048), so a draw whose target lies within 2^-40 * (row total) of any
entry of its row's CDF is AMBIGUOUS; a family with an ambiguous draw is left out of the comparison, every other family
must match exactly.  The share left out may not exceed 1e-4 in any case (about 4e7 draws at 4e-9 each: 0 is expected);
the seeds below meet that on the oracle's matrices, which the non-GPU test asserts for every case."""
import numpy as np
import pytest

from cafexp_amd import problem as P, synth
from test_simulate import _tree

U32 = np.uint64(0xFFFFFFFF)
AMBIGUOUS = 2.0 ** -40          # of the row total, either side of a CDF entry
LEFT_OUT = 1e-4                 # largest share of families an ambiguous draw may take out of a comparison


# ---------------------------------------------------------------------------------------------------- the replay
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """tree_sampler.h's philox4x32_10 on uint64 arrays that hold 32-bit words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & U32, (k1 + np.uint64(0xBB67AE85)) & U32
    return c0, c1, c2, c3


def uniform01(family, node, stream, seed):
    """tree_sampler.h's uniform01: counter (family lo, family hi, node, stream), key (seed lo, seed hi), 53 bits in (0, 1)."""
    family = np.asarray(family, dtype=np.uint64)
    r0, r1, _, _ = philox4x32_10(family & U32, family >> np.uint64(32), node, stream, seed & 0xFFFFFFFF, seed >> 32)
    return (((r0 << np.uint64(21)) ^ (r1 >> np.uint64(11))).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def draw(rows, u):
    """The child size of every family: rows[i] is the CDF row of its parent's size.  np.searchsorted(rows[i], target[i],
    side="left") for all i at once: in a non-decreasing row that index is the number of entries below the target.
    Returns (sizes, ambiguous)."""
    total = rows[:, -1]
    target = u * total
    size = (rows < target[:, None]).sum(axis=1)
    near = np.abs(rows - target[:, None]).min(axis=1) <= AMBIGUOUS * total
    return size, near & (total > 0)                          # an all-zero row gives 0 whatever the rounding


def replay(tree, lambdas, S, roots, seed, matrices, chunk_size=0, chunk_multiplier=None, error_model=None):
    """cafe_simulate on the host.  matrices(S, lambdas, ts) -> [len][S][S] row-major transition matrices.
    Returns (leaf_counts [F][n_taxa], node_sizes [F][n_nodes], ambiguous [F])."""
    F, n = len(roots), tree.n_nodes
    lam = np.atleast_1d(np.asarray(lambdas, dtype=np.float64))
    chunk = chunk_size if chunk_size > 0 else max(F, 1)
    mult = np.ones(F) if chunk_multiplier is None else np.asarray(chunk_multiplier, dtype=np.float64)[np.arange(F) // chunk]
    root = int(np.where(tree.parent < 0)[0][0])
    branches = [v for v in range(n) if v != root]
    sizes = np.zeros((F, n), dtype=np.int64)
    sizes[:, root] = roots
    ambiguous = np.zeros(F, dtype=bool)
    for m in np.unique(mult):                                # the families of the chunks that share a multiplier
        fam = np.where(mult == m)[0]
        mats = matrices(S, lam[tree.lambda_index[branches]] * m, tree.branch_length[branches])
        cdf = np.cumsum(mats[:, :, :S], axis=2)
        for v in sorted(branches, reverse=True):             # parents have larger indices: parents first
            ps = sizes[fam, tree.parent[v]]
            size, near = draw(cdf[branches.index(v)][ps], uniform01(fam, v, 0, seed))
            size[ps == 0] = 0                                # an extinct lineage stays extinct, no draw
            ambiguous[fam] |= near & (ps > 0)
            if error_model is not None and tree.leaf_taxon[v] >= 0:
                probs = error_model[size]
                u = uniform01(fam, v, 1, seed)
                down = u < probs[:, 0]
                size = size - down + (~down & (u > 1 - probs[:, 2]))
            sizes[fam, v] = size
    leaves = np.where(tree.leaf_taxon >= 0)[0]
    return sizes[:, leaves[np.argsort(tree.leaf_taxon[leaves])]], sizes, ambiguous


def _oracle_matrices(oracle):
    return lambda S, lams, ts: np.stack([oracle.build_matrix(S, float(l), float(t), fast=True) for l, t in zip(lams, ts)])


# ---------------------------------------------------------------------------------------------------- the cases
THREE_TAPS = [[0.0, 0.9, 0.1], [0.1, 0.8, 0.1]]
WIDE_S = [2, 3, 64, 65, 129, 751, 2048]
SHAPES = {
    "polytomy": "(A:15,B:22.5,C:7,(D:30,E:12):9);",          # also leaves under the root
    "leaf_under_root_tq0": "((A:0.0004,B:10):10,C:20);",     # A's branch quantizes to t_q = 0: all-zero rows
    "saturated_for_one_multiplier": "((A:40,B:10):12,(C:8,(D:25,E:5):6):3);",
}
SHAPE_LAMBDAS = [0.01, 0.004]
SHAPE_MULTIPLIERS = [1.0, 0.5, 2.6, 1.3]                     # 2.6 * 0.01 * 40 > 1: A's branch of the third tree saturates


def _error_model(S):
    return P.error_model_table(THREE_TAPS, S - 1)


def bench_case():
    """The bench's 100-taxon tree (199 nodes: the transposes take 2 and 4 column tiles), 20 011 families (not a multiple of
    64 or 256) in 47 chunks with gamma-like multipliers, 3-tap error model."""
    rng = np.random.default_rng(synth.DEFAULT_SEED)
    tree = _tree(text=synth.to_newick(synth.yule_tree(100, rng)))
    assert tree.n_taxa == 100 and tree.n_nodes == 199
    F, chunk = 20011, 426
    assert (F + chunk - 1) // chunk == 47 and F % 64 and F % 256 and chunk % 64
    return dict(tree=tree, lambdas=[0.002], S=100, roots=rng.integers(0, 100, F).astype(np.int32), seed=0x5EED0001CAFE,
                chunk_size=chunk, chunk_multiplier=rng.gamma(1.5, 1 / 1.5, 47), error_model=_error_model(100))


def wide_case(S):
    """Rows of S columns (row_cdf: a partial block, many blocks; K1 at its narrowest and widest E), root sizes over 0..S-1."""
    rng = np.random.default_rng(S)
    F = 4113
    roots = rng.permutation(np.arange(F) % S).astype(np.int32)
    assert set(roots) == set(range(S))
    return dict(tree=_tree(text="((A:7.25,B:23.904):61.337,C:9.75);"), lambdas=[0.002], S=S, roots=roots, seed=1000003 * S + 17)


def shape_case(name):
    """Two lambdas through lambda_index, chunks of 50 families over four multipliers, 3-tap error model."""
    tree = _tree(text=SHAPES[name])
    tree.lambda_index = (np.arange(tree.n_nodes) % 2).astype(np.int32)
    F = 6000
    rng = np.random.default_rng(len(name))
    return dict(tree=tree, lambdas=SHAPE_LAMBDAS, S=100, roots=rng.integers(0, 100, F).astype(np.int32), seed=(7 << 32) + len(name),
                chunk_size=50, chunk_multiplier=np.array(SHAPE_MULTIPLIERS)[np.arange(F // 50) % 4], error_model=_error_model(100))


CASES = [("bench", bench_case, ())] + [("wide%d" % S, wide_case, (S,)) for S in WIDE_S] + [(nm, shape_case, (nm,)) for nm in SHAPES]


def _simulate(capi, case, **kw):
    em = case.get("error_model")
    return capi.simulate(case["tree"], case["lambdas"], case["S"], case["roots"], seed=case["seed"], chunk_size=case.get("chunk_size", 0),
                         chunk_multiplier=case.get("chunk_multiplier"), error_model=em, error_model_max_size=case["S"] if em is not None else 0, **kw)


def _replay(case, matrices):
    return replay(case["tree"], case["lambdas"], case["S"], case["roots"], case["seed"], matrices, chunk_size=case.get("chunk_size", 0),
                  chunk_multiplier=case.get("chunk_multiplier"), error_model=case.get("error_model"))


def _compare(name, device, replayed):
    """Equality family by family, the families with an ambiguous draw left out (at most LEFT_OUT of them)."""
    (d_leaf, d_nodes), (r_leaf, r_nodes, ambiguous) = device, replayed
    F = len(ambiguous)
    keep = ~ambiguous
    print("%s: %d families compared, %d left out" % (name, keep.sum(), ambiguous.sum()))
    assert ambiguous.sum() <= LEFT_OUT * F
    bad = np.where(keep & ((d_nodes != r_nodes).any(axis=1) | (d_leaf != r_leaf).any(axis=1)))[0]
    assert len(bad) == 0, "%s: %d families differ, first %d: device %s replay %s" % (name, len(bad), bad[0], d_nodes[bad[0]], r_nodes[bad[0]])


# ---------------------------------------------------------------------------------------------------- CPU
KNOWN_ANSWERS = [                                            # Philox4x32-10, the generator's published test vectors
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        assert tuple(int(w) for w in philox4x32_10(*ctr, *key)) == want
    ctrs = np.array([k[0] for k in KNOWN_ANSWERS], dtype=np.uint64).T      # vectorised: one lane per vector
    keys = np.array([k[1] for k in KNOWN_ANSWERS], dtype=np.uint64).T
    assert np.array_equal(np.array(philox4x32_10(*ctrs, *keys)).T, np.array([k[2] for k in KNOWN_ANSWERS], dtype=np.uint64))


def test_uniform_and_draw():
    u = uniform01(np.arange(100000), 7, 1, (5 << 32) + 9)
    assert u.min() > 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.005
    r0, r1, _, _ = philox4x32_10(3, 0, 7, 1, 9, 5)           # family 3, node 7, stream 1, seed (5 << 32) + 9
    assert u[3] == (float((int(r0) << 21) ^ (int(r1) >> 11)) + 0.5) / 2.0 ** 53
    rng = np.random.default_rng(0)
    rows = np.cumsum(rng.random((500, 37)) * (rng.random((500, 37)) < 0.7), axis=1)      # rows with runs of equal entries
    rows[:5] = 0
    uu = rng.random(500)
    uu[5:10] = [0.0, 1.0, 0.5, 0.25, 0.75]
    size, near = draw(rows, uu)
    want = [np.searchsorted(rows[i], uu[i] * rows[i, -1], side="left") for i in range(500)]
    assert np.array_equal(size, want) and not size[:5].any() and not near[:5].any()
    exact = np.cumsum(np.ones((1, 8)), axis=1)               # a target on an entry is ambiguous, one between entries is not
    assert draw(exact, np.array([0.5]))[1][0] and not draw(exact, np.array([0.55]))[1][0]


@pytest.mark.parametrize("name,make,args", CASES, ids=[c[0] for c in CASES])
def test_seeds_leave_no_family_out_on_the_oracle_matrices(oracle, name, make, args):
    """The condition of the GPU comparison, checked without a GPU: the replay over the oracle's matrices marks at most
    LEFT_OUT of a case's families ambiguous (0 expected)."""
    case = make(*args)
    tree = case["tree"]
    leaf, nodes, ambiguous = _replay(case, _oracle_matrices(oracle))
    F, S = len(ambiguous), case["S"]
    print("%s: %d of %d families hold an ambiguous draw" % (name, ambiguous.sum(), F))
    assert ambiguous.sum() <= LEFT_OUT * F
    root = int(np.where(tree.parent < 0)[0][0])
    assert np.array_equal(nodes[:, root], case["roots"]) and nodes.min() >= 0 and nodes.max() <= S
    assert not nodes[case["roots"] == 0][:, tree.leaf_taxon < 0].any()      # extinct at the root: extinct at every interior node
    assert leaf.shape == (F, tree.n_taxa) and (nodes.std(axis=0) > 0).sum() >= 2


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


@pytest.mark.gpu
def test_bench_tree_replayed(capi):
    """199 nodes and 100 taxa (4 and 2 column tiles per transpose), 47 chunks; under the automatic workspace, a 1-byte limit
    (64 families and one matrix block per batch: a chunk runs on over batch ends) and 16 MB."""
    case = bench_case()
    replayed = _replay(case, capi.build_matrices)
    for limit in (0, 1, 16 << 20):
        _compare("bench tree, workspace limit %d" % limit, _simulate(capi, case, workspace_limit=limit), replayed)


@pytest.mark.gpu
@pytest.mark.parametrize("S", WIDE_S)
def test_wide_rows_replayed(capi, S):
    case = wide_case(S)
    _compare("S = %d" % S, _simulate(capi, case), _replay(case, capi.build_matrices))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_tree_shapes_replayed(capi, name):
    case = shape_case(name)
    tree = case["tree"]
    br = np.where(tree.parent >= 0)[0]
    zero = {}                                                # per multiplier: the branches whose matrix has all-zero rows s >= 1
    for m in SHAPE_MULTIPLIERS:
        mats = capi.build_matrices(100, np.array(SHAPE_LAMBDAS)[tree.lambda_index[br]] * m, tree.branch_length[br])
        zero[m] = {int(v) for v, mat in zip(br, mats) if not mat[1:].any()}
    if name == "saturated_for_one_multiplier":
        a = int(np.where(tree.leaf_taxon == 0)[0][0])
        assert tree.branch_length[a] == 40 and zero[2.6] == {a} and not zero[1.0] and not zero[0.5] and not zero[1.3]
    if name == "leaf_under_root_tq0":
        assert all(len(z) == 1 for z in zero.values())
    assert set(tree.lambda_index[br]) == {0, 1}
    _compare(name, _simulate(capi, case), _replay(case, capi.build_matrices))
