"""Gene-family simulation: the reference's -s (src/simulator.cpp, src/probability.cpp:320-377).

CPU: the driver's argument refusals (no device touched).
GPU: the cafexp_hip driver's host path -- draws that consume the engine like the reference, matrices from
cafe_build_matrices -- against the reference's own output files at seed 10 (tests/golden/ref_simulate.json, written by
tests/golden/make_simulate_golden.py); cafe_simulate's device sampler against the exact marginals of the model
(chi-square per node), its determinism across seeds and workspace limits, its edge cases, and a simulate-then-estimate
round trip through the driver.
"""
import json
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest

from cafexp_amd import capi, problem as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
DATA = os.path.join(ROOT, "tests", "golden", "data")
S = 100                                                    # the simulator's matrix order without -f (simulator.cpp:70)


def _driver(args, timeout=600):
    assert os.path.exists(EXE), "cafexp_hip missing: run __graft_entry__.build()"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def _our_args(ref_args):
    """The reference's command line in the driver's terms: -sN -> --simulate N (-s is the SEED here), data paths."""
    out = []
    for i, a in enumerate(ref_args):
        if a.startswith("-s"):
            out += ["--simulate"] + ([a[2:]] if a[2:] else [])
        elif i > 0 and ref_args[i - 1] in ("-t", "-f", "-y", "-e"):
            out.append(os.path.join(DATA, a))
        else:
            out.append(a)
    return out


def _tree(name="mammals_tree.txt", text=None):
    """Flattened tree (post order: children before parents) in the shape capi.simulate reads."""
    root = P.parse_newick(text if text is not None else open(os.path.join(DATA, name)).read())
    nodes = root.postorder()
    index = {id(n): i for i, n in enumerate(nodes)}
    leaves = [n for n in nodes if n.is_leaf]
    col = {id(l): j for j, l in enumerate(leaves)}
    return types.SimpleNamespace(
        n_nodes=len(nodes), n_taxa=len(leaves),
        parent=np.array([index[id(n.parent)] if n.parent is not None else -1 for n in nodes], dtype=np.int32),
        branch_length=np.array([n.length for n in nodes]),
        lambda_index=np.zeros(len(nodes), dtype=np.int32),
        leaf_taxon=np.array([col.get(id(n), -1) for n in nodes], dtype=np.int32))


def _transitions(lam, tree, mult):
    """Per node, the sampler's transition rows: row s of the order-S matrix over 0..S-1, normalised; parent 0 and
    all-zero rows give 0."""
    br = [v for v in range(tree.n_nodes) if tree.parent[v] >= 0]
    mats = capi.build_matrices(S, np.full(len(br), lam * mult), tree.branch_length[br])
    out = {}
    for v, m in zip(br, mats):
        w = m[:, :S].copy()
        tot = w.sum(axis=1)
        zero = ~(tot > 0)
        w[~zero] /= tot[~zero, None]
        w[zero] = 0
        w[zero, 0] = 1
        w[0] = 0
        w[0, 0] = 1
        out[v] = w
    return out


def _marginals(tree, roots, trans, em=None):
    """Exact distribution of every node's size given the root sizes; leaves convolved with the error model.
    Index i of a leaf's vector is size i - 1 (sizes -1..S)."""
    p = [None] * tree.n_nodes
    root = int(np.where(tree.parent < 0)[0][0])
    p[root] = np.bincount(roots, minlength=S)[:S] / len(roots)
    for v in range(tree.n_nodes - 1, -1, -1):              # parents have larger indices
        if v != root:
            p[v] = p[tree.parent[v]][:S] @ trans[v]
    out = []
    for v in range(tree.n_nodes):
        q = np.zeros(S + 2)
        q[1:S + 1] = p[v][:S]
        if em is not None and tree.leaf_taxon[v] >= 0:
            r = np.zeros(S + 2)
            for c in range(S):
                lo, hi = em[c, 0], em[c, 2]
                r[c] += q[c + 1] * lo
                r[c + 2] += q[c + 1] * hi
                r[c + 1] += q[c + 1] * (1 - lo - hi)
            q = r
        out.append(q)
    return out


def _chi2_p(observed, expected):
    """Goodness of fit with bins pooled (in size order) until each holds an expectation >= 5."""
    from scipy.stats import chi2
    o_b, e_b, o_acc, e_acc = [], [], 0.0, 0.0
    for o, e in zip(observed, expected):
        o_acc += o
        e_acc += e
        if e_acc >= 5:
            o_b.append(o_acc)
            e_b.append(e_acc)
            o_acc = e_acc = 0.0
    if e_b:
        o_b[-1] += o_acc
        e_b[-1] += e_acc
    o_b, e_b = np.array(o_b), np.array(e_b)
    if len(e_b) < 2:
        return 1.0 if abs(o_b.sum() - e_b.sum()) < 1e-6 * max(1, e_b.sum()) else 0.0
    return float(chi2.sf(((o_b - e_b) ** 2 / e_b).sum(), len(e_b) - 1))


def _error_model(name="errormodel_600.txt"):
    _, _, dists = P.read_error_model(open(os.path.join(DATA, name)).read())
    return P.error_model_table(dists, S - 1), len(dists)


MULTS = np.array([0.3, 0.8, 1.2, 2.5])                     # 2.5 * 0.01 * 96.4 > 1: mammals' longest branch saturates


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("extra,message", [
    (["-i", os.path.join(DATA, "mammal_gene_families.txt"), "-f", os.path.join(DATA, "rootdist_small.txt"), "-l", "0.01"],
     "Options -i and -f are mutually exclusive."),
    (["-k", "3", "-l", "0.01"], "Cannot simulate gamma clusters without an alpha value"),
    (["-k", "3", "-a", "-1", "-l", "0.01"], "Cannot simulate gamma clusters without an alpha value"),
    ([], "Cannot simulate without initial lambda values"),
])
def test_driver_refuses_bad_simulation_arguments(extra, message):
    with tempfile.TemporaryDirectory() as tmp:
        p = _driver(["-t", os.path.join(DATA, "mammals_tree.txt"), "--simulate", "10", "-o", tmp] + extra, timeout=120)
        assert p.returncode == 1, (p.stdout, p.stderr)
        assert message in p.stderr
        assert not os.path.exists(os.path.join(tmp, "simulation.txt"))


def test_golden_fixture_covers_the_contract():
    with open(os.path.join(ROOT, "tests", "golden", "ref_simulate.json")) as f:
        g = json.load(f)["cases"]
    assert g["gamma"]["simulation.txt"].count("\n") == 261 and g["gamma"]["average_multiplier"] not in (None, "-nan")
    assert g["base"]["average_multiplier"] == "-nan" and g["multi_lambda"]["average_multiplier"] is None
    assert g["rootdist_full"]["simulation.txt"].count("\n") == 15 and g["rootdist_pared"]["simulation.txt"].count("\n") == 41
    assert g["error_model_too_small"]["rc"] == 1
    header = g["base"]["simulation_truth.txt"].split("\n")[0].split("\t")
    assert len(header) == 2 + 23 and header[5] == "3"


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def sim_golden():
    with open(os.path.join(ROOT, "tests", "golden", "ref_simulate.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["base", "gamma", "rootdist_pared", "rootdist_full", "error_model", "multi_lambda", "error_model_too_small"])
def test_host_path_reproduces_the_reference(sim_golden, case):
    """cafexp_hip --simulate at seed 10 writes the reference's files byte for byte (draw for draw on the same engine)."""
    c = sim_golden[case]
    with tempfile.TemporaryDirectory() as tmp:
        p = _driver(_our_args(c["args"]) + ["-s", "10", "-o", tmp])
        assert p.returncode == c["rc"], (p.stdout, p.stderr)
        if c["rc"]:
            assert c["message"] in p.stderr
            return
        avg = [l.split(": ", 1)[1] for l in p.stdout.splitlines() if l.startswith("Average multiplier for simulated values: ")]
        assert (avg[0] if avg else None) == c["average_multiplier"]
        for name in ("simulation.txt", "simulation_truth.txt"):
            got = open(os.path.join(tmp, name)).read()
            if got != c[name]:
                gl, wl = got.splitlines(), c[name].splitlines()
                bad = [i for i in range(min(len(gl), len(wl))) if gl[i] != wl[i]]
                pytest.fail("%s: %d lines differ, first %s\n got  %s\n want %s" % (name, len(bad), bad[:5], gl[bad[0]] if bad else "", wl[bad[0]] if bad else ""))
        info = json.loads(p.stdout.strip().splitlines()[-1])
        assert info["mode"] == "host" and info["n_families"] == c["simulation.txt"].count("\n") - 1
        if case == "gamma":                                # some chunk saturates mammals' longest branch (96.4)
            assert len(info["multipliers"]) == 6 and max(info["multipliers"]) > 1 / (0.01 * 96.435575)


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [False, True])
@pytest.mark.parametrize("with_em", [False, True])
def test_device_marginals(gamma, with_em):
    """cafe_simulate's families follow the model: per node, chi-square against the exact marginal (p > 1e-4)."""
    tree = _tree()
    F, chunk, lam = 200_000, 50, 0.01
    rng = np.random.default_rng(11)
    roots = rng.integers(0, S, F).astype(np.int32)
    mult = MULTS[rng.integers(0, len(MULTS), F // chunk)] if gamma else None
    em, em_max = _error_model() if with_em else (None, 0)
    leaf, nodes = capi.simulate(tree, [lam], S, roots, seed=1234, chunk_size=chunk, chunk_multiplier=mult,
                                error_model=em, error_model_max_size=em_max)
    groups = [(np.arange(F), 1.0)] if not gamma else [(np.where(np.repeat(mult, chunk) == m)[0], m) for m in MULTS]
    expected = [np.zeros(S + 2) for _ in range(tree.n_nodes)]
    for fams, m in groups:
        marg = _marginals(tree, roots[fams], _transitions(lam, tree, m), em)
        for v in range(tree.n_nodes):
            expected[v] += marg[v] * len(fams)
    worst = 1.0
    for v in range(tree.n_nodes):
        obs = np.bincount(nodes[:, v] + 1, minlength=S + 2)
        assert len(obs) == S + 2 and obs.sum() == F
        pv = _chi2_p(obs, expected[v])
        worst = min(worst, pv)
        assert pv > 1e-4, (v, pv)
    print("worst node p-value %.3g" % worst)


@pytest.mark.gpu
def test_device_conditional_on_parent():
    """The longest leaf branch: the child sizes drawn under each frequent parent size follow that row of the matrix."""
    tree = _tree()
    F, lam = 200_000, 0.01
    roots = np.random.default_rng(5).integers(1, 40, F).astype(np.int32)
    _, nodes = capi.simulate(tree, [lam], S, roots, seed=77)
    trans = _transitions(lam, tree, 1.0)
    v = int(np.argmax(tree.branch_length * (tree.leaf_taxon >= 0)))     # the longest leaf branch
    par = nodes[:, tree.parent[v]]
    sizes, counts = np.unique(par, return_counts=True)
    tested = 0
    for s in sizes[np.argsort(-counts)][:6]:
        sel = nodes[par == s, v]
        pv = _chi2_p(np.bincount(sel, minlength=S)[:S], trans[v][s] * len(sel))
        assert pv > 1e-4, (s, pv)
        tested += 1
    assert tested == 6


@pytest.mark.gpu
def test_device_determinism_and_batching():
    tree = _tree()
    F, chunk = 20_000, 50
    rng = np.random.default_rng(3)
    roots = rng.integers(0, S, F).astype(np.int32)
    mult = rng.gamma(1.5, 1 / 1.5, F // chunk)
    em, em_max = _error_model()
    kw = dict(chunk_size=chunk, chunk_multiplier=mult, error_model=em, error_model_max_size=em_max)
    a_leaf, a_nodes = capi.simulate(tree, [0.01], S, roots, seed=42, **kw)
    b_leaf, b_nodes = capi.simulate(tree, [0.01], S, roots, seed=42, **kw)
    assert np.array_equal(a_leaf, b_leaf) and np.array_equal(a_nodes, b_nodes)
    c_leaf, _ = capi.simulate(tree, [0.01], S, roots, seed=43, **kw)
    assert (c_leaf != a_leaf).mean() > 0.5
    # 1 byte: one matrix block and 64 families per batch (313 batches); 16 MB: a few blocks per batch
    for limit in (1, 16 << 20):
        d_leaf, d_nodes = capi.simulate(tree, [0.01], S, roots, seed=42, workspace_limit=limit, **kw)
        assert np.array_equal(d_leaf, a_leaf) and np.array_equal(d_nodes, a_nodes), limit
    leaf_only, none = capi.simulate(tree, [0.01], S, roots, seed=42, node_sizes=False, **kw)
    assert none is None and np.array_equal(leaf_only, a_leaf)
    leaves = np.where(tree.leaf_taxon >= 0)[0]
    assert np.array_equal(a_nodes[:, leaves[np.argsort(tree.leaf_taxon[leaves])]], a_leaf)
    root = int(np.where(tree.parent < 0)[0][0])
    assert np.array_equal(a_nodes[:, root], roots)


@pytest.mark.gpu
def test_device_edges():
    tree = _tree()
    leaf, nodes = capi.simulate(tree, [0.01], S, np.zeros(1000, dtype=np.int32), seed=1)
    assert not leaf.any() and not nodes.any()                                  # extinct at the root: extinct everywhere
    sat = _tree(text="(A:200,B:1);")                                           # 0.01 * 200 > 1: A's branch saturates
    leaf, nodes = capi.simulate(sat, [0.01], S, np.full(1000, 5, dtype=np.int32), seed=1)
    a = list(sat.leaf_taxon).index(0)
    assert not nodes[:, a].any() and nodes[:, 1 - a].std() > 0
    em, _ = _error_model()
    with pytest.raises(capi.CafeError, match="Trying to simulate leaf family size that was not included in error model"):
        capi.simulate(tree, [0.01], S, np.full(100, 50, dtype=np.int32), seed=1, error_model=em, error_model_max_size=3)
    roots = np.ones(10, dtype=np.int32)
    for lam in (-0.01, float("nan"), 0.0):
        with pytest.raises(capi.CafeError, match="invalid lambda"):
            capi.simulate(tree, [lam], S, roots, seed=1)
    with pytest.raises(capi.CafeError, match="matrix order"):
        capi.simulate(tree, [0.01], 2049, roots, seed=1)
    with pytest.raises(capi.CafeError, match="root size"):
        capi.simulate(tree, [0.01], S, np.full(10, S, dtype=np.int32), seed=1)


@pytest.mark.gpu
def test_simulate_then_estimate_round_trip():
    """20 000 device-simulated base-model families at lambda 0.01, read back by the estimator: lambda-hat within 20 %.
    The simulator's rows stop at size 99 (S = 100, as the reference's) while its root sizes reach 99: a parent of 90
    loses ~20 % of its row's mass above 99 on mammals' longest branches, which narrows the spread of the large families
    and pulls lambda-hat low (observed: 0.00858, -14 %).  The sampler itself is pinned to the exact
    model by test_device_marginals."""
    tree = os.path.join(DATA, "mammals_tree.txt")
    with tempfile.TemporaryDirectory() as tmp:
        p = _driver(["-t", tree, "-l", "0.01", "--simulate", "20000", "--simulate-device", "-s", "3", "-o", tmp])
        assert p.returncode == 0, p.stderr
        info = json.loads(p.stdout.strip().splitlines()[-1])
        assert info["mode"] == "device" and info["n_families"] == 20000
        for name in ("simulation.txt", "simulation_truth.txt"):
            lines = open(os.path.join(tmp, name)).read().splitlines()
            assert len(lines) == 20001 and lines[1].startswith("NULL\tsimfam0\t")
        est = _driver(["-t", tree, "-i", os.path.join(tmp, "simulation.txt")])
        assert est.returncode == 0, est.stderr
        lam = json.loads(est.stdout.strip().splitlines()[-1])["lambda"][0]
        print("lambda-hat %.6f (relative error %.3f)" % (lam, abs(lam - 0.01) / 0.01))
        assert abs(lam - 0.01) / 0.01 < 0.20
