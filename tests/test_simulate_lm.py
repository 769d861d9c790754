"""cafe_simulate_lm: the device simulator under separate birth and death rates, replayed draw for draw on the host.

tests/test_simulate_replay.py states the sampler in numpy (Philox counters, uniform01, the inverse-CDF draw, the error-model step)
and its rule for a draw that the two summation orders may round differently (AMBIGUOUS; at most LEFT_OUT of a case's families,
a condition and not a measurement).  Here its branch loop is restated with one (lambda, mu) per lambda index over the rows of
capi.build_matrices_lm -- a chunk multiplier scales both rates -- and the device's leaf counts and node sizes must be EQUAL family
by family.  The non-GPU test asserts the condition for every case and seed on the matrices of tests/bd_lm_ref.py."""
import numpy as np
import pytest

import bd_lm_ref as R
from test_simulate import _tree
from test_simulate_replay import AMBIGUOUS, LEFT_OUT, SHAPE_LAMBDAS, SHAPE_MULTIPLIERS, SHAPES, _error_model, draw, uniform01

assert AMBIGUOUS == 2.0 ** -40 and LEFT_OUT == 1e-4
WIDE_S = [2, 65, 751, 2048]
MU_OVER_LAMBDA = [0.6, 1.7]
SHAPE_NAMES = ["polytomy", "saturated_for_one_multiplier"]


def replay_lm(tree, lambdas, mus, S, roots, seed, matrices, chunk_size=0, chunk_multiplier=None, error_model=None):
    """test_simulate_replay.replay with a death rate per lambda index.  matrices(S, lambdas, mus, ts) -> [len][S][S]."""
    F, n = len(roots), tree.n_nodes
    lam, mu = np.atleast_1d(np.asarray(lambdas, dtype=np.float64)), np.atleast_1d(np.asarray(mus, dtype=np.float64))
    chunk = chunk_size if chunk_size > 0 else max(F, 1)
    mult = np.ones(F) if chunk_multiplier is None else np.asarray(chunk_multiplier, dtype=np.float64)[np.arange(F) // chunk]
    root = int(np.where(tree.parent < 0)[0][0])
    branches = [v for v in range(n) if v != root]
    sizes = np.zeros((F, n), dtype=np.int64)
    sizes[:, root] = roots
    ambiguous = np.zeros(F, dtype=bool)
    for m in np.unique(mult):
        fam = np.where(mult == m)[0]
        idx = tree.lambda_index[branches]
        mats = matrices(S, lam[idx] * m, mu[idx] * m, tree.branch_length[branches])      # the multiplier scales both rates
        cdf = np.cumsum(mats[:, :, :S], axis=2)
        for v in sorted(branches, reverse=True):             # parents first
            ps = sizes[fam, tree.parent[v]]
            size, near = draw(cdf[branches.index(v)][ps], uniform01(fam, v, 0, seed))
            size[ps == 0] = 0
            ambiguous[fam] |= near & (ps > 0)
            if error_model is not None and tree.leaf_taxon[v] >= 0:
                probs = error_model[size]
                u = uniform01(fam, v, 1, seed)
                down = u < probs[:, 0]
                size = size - down + (~down & (u > 1 - probs[:, 2]))
            sizes[fam, v] = size
    leaves = np.where(tree.leaf_taxon >= 0)[0]
    return sizes[:, leaves[np.argsort(tree.leaf_taxon[leaves])]], sizes, ambiguous


def wide_case(S, ratio):
    rng = np.random.default_rng(S)
    F = 4113
    roots = rng.permutation(np.arange(F) % S).astype(np.int32)
    return dict(tree=_tree(text="((A:7.25,B:23.904):61.337,C:9.75);"), lambdas=[0.002], mus=[0.002 * ratio], S=S, roots=roots,
                seed=1000003 * S + 17 + int(10 * ratio))


def shape_case(name, ratio):
    tree = _tree(text=SHAPES[name])
    tree.lambda_index = (np.arange(tree.n_nodes) % 2).astype(np.int32)
    F = 6000
    rng = np.random.default_rng(len(name))
    return dict(tree=tree, lambdas=SHAPE_LAMBDAS, mus=[ratio * v for v in SHAPE_LAMBDAS], S=100, roots=rng.integers(0, 100, F).astype(np.int32),
                seed=(11 << 32) + len(name) + int(10 * ratio), chunk_size=50,
                chunk_multiplier=np.array(SHAPE_MULTIPLIERS)[np.arange(F // 50) % 4], error_model=_error_model(100))


CASES = [("wide%d_mu%g" % (S, r), wide_case, (S, r)) for S in WIDE_S for r in MU_OVER_LAMBDA] + \
        [("%s_mu%g" % (nm, r), shape_case, (nm, r)) for nm in SHAPE_NAMES for r in MU_OVER_LAMBDA]


def _simulate(capi, case, mus="case", **kw):
    em = case.get("error_model")
    return capi.simulate_lm(case["tree"], case["lambdas"], case["mus"] if isinstance(mus, str) else mus, case["S"], case["roots"],
                            seed=case["seed"], chunk_size=case.get("chunk_size", 0), chunk_multiplier=case.get("chunk_multiplier"),
                            error_model=em, error_model_max_size=case["S"] if em is not None else 0, **kw)


def _replay(case, matrices):
    return replay_lm(case["tree"], case["lambdas"], case["mus"], case["S"], case["roots"], case["seed"], matrices,
                     chunk_size=case.get("chunk_size", 0), chunk_multiplier=case.get("chunk_multiplier"), error_model=case.get("error_model"))


def _numpy_matrices(S, lams, mus, ts):
    return np.stack([R.matrix(S, float(l), float(m), float(t)) for l, m, t in zip(lams, mus, ts)])


def _compare(name, device, replayed):
    (d_leaf, d_nodes), (r_leaf, r_nodes, ambiguous) = device, replayed
    F = len(ambiguous)
    keep = ~ambiguous
    print("%s: %d families compared, %d left out" % (name, keep.sum(), ambiguous.sum()))
    assert ambiguous.sum() <= LEFT_OUT * F
    bad = np.where(keep & ((d_nodes != r_nodes).any(axis=1) | (d_leaf != r_leaf).any(axis=1)))[0]
    assert len(bad) == 0, "%s: %d families differ, first %d: device %s replay %s" % (name, len(bad), bad[0], d_nodes[bad[0]], r_nodes[bad[0]])


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name,make,args", CASES, ids=[c[0] for c in CASES])
def test_seeds_leave_no_family_out_on_the_numpy_matrices(name, make, args):
    case = make(*args)
    tree = case["tree"]
    leaf, nodes, ambiguous = _replay(case, _numpy_matrices)
    F, S = len(ambiguous), case["S"]
    print("%s: %d of %d families hold an ambiguous draw" % (name, ambiguous.sum(), F))
    assert ambiguous.sum() <= LEFT_OUT * F
    root = int(np.where(tree.parent < 0)[0][0])
    assert np.array_equal(nodes[:, root], case["roots"]) and nodes.min() >= 0 and nodes.max() <= S
    assert leaf.shape == (F, tree.n_taxa)
    if name.startswith("saturated"):
        # coeff = 1 - alpha - beta < 0 needs (lambda + mu) t / 2 beyond about 1: with mu = 1.7 lambda A's branch (t = 40) still
        # saturates for the multiplier 2.6 only, with mu = 0.6 lambda for none -- the shape then runs as an ordinary tree
        a = int(np.where(tree.leaf_taxon == 0)[0][0])
        lam, mu = case["lambdas"][tree.lambda_index[a]], case["mus"][tree.lambda_index[a]]
        assert [R.rates(lam * m, mu * m, 40.0)[2] for m in SHAPE_MULTIPLIERS] == [False, False, args[1] > 1, False]


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def capi():
    from cafexp_amd import capi as C
    C.load()
    return C


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,args", CASES, ids=[c[0] for c in CASES])
def test_replayed_draw_for_draw(capi, name, make, args):
    case = make(*args)
    _compare(name, _simulate(capi, case), _replay(case, capi.build_matrices_lm))


@pytest.mark.gpu
def test_null_and_equal_rates_are_cafe_simulate(capi):
    for case in (wide_case(65, 1.0), shape_case("polytomy", 1.0)):
        em = case.get("error_model")
        plain = capi.simulate(case["tree"], case["lambdas"], case["S"], case["roots"], seed=case["seed"], chunk_size=case.get("chunk_size", 0),
                              chunk_multiplier=case.get("chunk_multiplier"), error_model=em, error_model_max_size=case["S"] if em is not None else 0)
        assert case["mus"] == list(case["lambdas"])
        for mus in (None, case["mus"]):
            got = _simulate(capi, case, mus=mus)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), mus
        other = _simulate(capi, case, mus=[0.5 * v for v in case["lambdas"]])
        assert not np.array_equal(other[1], plain[1])


@pytest.mark.gpu
def test_the_batches_do_not_matter(capi):
    case = shape_case("polytomy", 0.6)
    whole = _simulate(capi, case)
    cut = _simulate(capi, case, workspace_limit=1)           # 64 families and one matrix block per batch: >= 94 batches
    assert len(case["roots"]) >= 3 * 64
    assert np.array_equal(whole[0], cut[0]) and np.array_equal(whole[1], cut[1])


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [-1e-9, float("nan"), float("inf"), 2e9])
def test_an_invalid_mu_is_an_argument_error(capi, bad):
    case = wide_case(65, 0.6)
    with pytest.raises(capi.CafeError, match=r"code 1: .*mu"):
        _simulate(capi, case, mus=[bad])


@pytest.mark.gpu
def test_pure_death_and_pure_birth_are_exact(capi):
    """A lambda below the key's quantum (1e-9) is valid (> 0) and quantizes to 0: pure death, whose matrix is exactly zero above
    the diagonal, so no child can exceed its parent; mu = 0 is pure birth, exactly zero below the diagonal."""
    tree = _tree(text="((A:30,B:30):30,C:30);")
    rng = np.random.default_rng(3)
    roots = rng.integers(1, 21, 4096).astype(np.int32)
    par = tree.parent
    br = np.where(par >= 0)[0]
    _, nodes = capi.simulate_lm(tree, [1e-10], [0.01], 200, roots, seed=99, chunk_size=0)
    assert np.all(nodes[:, br] <= nodes[:, par[br]])
    assert np.any(nodes[:, br] < nodes[:, par[br]])
    _, nodes = capi.simulate_lm(tree, [0.01], [0.0], 200, roots, seed=99, chunk_size=0)
    assert np.all(nodes[:, br] >= nodes[:, par[br]])
    assert np.any(nodes[:, br] > nodes[:, par[br]])
