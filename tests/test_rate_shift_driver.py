"""cafexp_hip --rate-shift-scan on synth20: with lambda searched, with -k 3 (lambda and alpha searched), with --estimate-mu
(lambda and mu searched: the 2-df test on birth and death) and with a two-lambda tree (-y: the clade of all branches under
lambda 2 is collinear with lambda 2 itself, so its clade row is not testable).

Every number of <Model>_rate_shift_scan.tab is recomputed in numpy (branch_scores_ref.score_test / holm) from the binding's
own cafe_branch_scores total and Gram matrix (CAFE_ROOT_MAX) at the printed optimum, to 1e-8 -- the tolerance of
test_standard_errors_driver.py -- relative to the number itself; U, which passes through zero, to 1e-8 of its standard
deviation sqrt(a^T G a), and V with 1e-12 a^T G a on top, the rounding of the subtraction that forms it.  The rows marked
"not testable" are the ones numpy finds, and NaN.  The lambda-tree file (written when the smallest Holm-adjusted clade p is
below -P; -P 1.1 makes that certain) parses as a lambda tree and labels that clade 2 and the rest 1."""
import json
import os
import subprocess

import numpy as np
import pytest

import branch_scores_ref as BR
import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import DATA, read, table
from test_events_driver import _reverse_level_order

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
COMMON = ["-t", os.path.join(DATA, "synth20_tree.txt"), "-i", os.path.join(DATA, "synth20_families.txt"), "-s", "7", "--rate-shift-scan"]
LAMBDA_TREE = os.path.join(DATA, "synth20_lambda_tree.txt")
COLUMNS = ["U", "V", "T", "P", "HolmP", "Multiplier"]


def _read(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# Score tests of a rate shift") and lines[1].startswith("#Node\t")
    return lines[0], lines[1][1:].split("\t"), [ln.split("\t") for ln in lines[2:]]


def _node_names(pb, species, order):
    names = {}
    for i, v in enumerate(order):
        names[v] = "%s<%d>" % (species[pb.leaf_taxon[v]], i) if pb.leaf_taxon[v] >= 0 else "<%d>" % i
    return names


def _close(got, want, floor=0.0):
    return abs(got - want) <= 1e-8 * abs(want) + floor


@pytest.mark.gpu
@pytest.mark.parametrize("extra,model,profiled", [([], "Base", ["Lambda"]), (["-k", "3"], "Gamma", ["Lambda", "Alpha"]),
                                                  (["--estimate-mu"], "Base", ["Lambda", "Mu"]),
                                                  (["-y", LAMBDA_TREE, "-P", "1.1"], "Base", ["Lambda1", "Lambda2"])])
def test_the_table_is_the_score_test_of_the_bindings_gram_matrix(tmp_path, extra, model, profiled):
    from cafexp_amd import capi
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([DRIVER] + COMMON + ["-o", str(tmp_path)] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    info = js["rate_shift_scan"]
    assert info["profiled"] == profiled and info["left_out"] == 0

    species, ids, counts = table("synth20_families.txt")
    lam_tree = P.parse_newick(read("synth20_lambda_tree.txt"), lambda_tree=True) if "-y" in extra else None
    pb = P.build_problem(P.parse_newick(read("synth20_tree.txt")), species, ids, counts, lambda_tree=lam_tree)
    assert pb.n_families == js["n_families"] == info["families"] and pb.max_family_size == js["max_family_size"]
    pr = P.Params(lambdas=np.array(js["lambda"]), prior=P.prior_uniform(pb.max_root_family_size))
    K = 1
    if model == "Gamma":
        K = 3
        pr.multipliers, pr.cat_probs = np.array(js["multipliers"]), np.full(3, 1.0 / 3)
    ctx = capi.Context(pb, max_categories=K)
    try:
        if "mu" in js:
            ctx.set_death_rates(js["mu"])
        got = ctx.branch_scores(pr, "max", alpha=js.get("alpha", 1.0), per_family=False)
    finally:
        ctx.close()
    assert not got["failed"].any()
    U, G = got["total"], got["gram"]
    Pdim, n_par, nl, nb = len(U), 2 if "mu" in js else 1, pb.n_lambdas, pb.n_nodes - 1
    glob = n_par * nb
    cols = [np.eye(Pdim)[:, glob + i] for i in range(nl)]
    if "mu" in js:
        cols += [np.eye(Pdim)[:, glob + nl + i] for i in range(nl)]
    if model == "Gamma":
        a = np.zeros(Pdim)
        a[glob + nl * n_par:] = info["dmultiplier_dalpha"]
        cols.append(a)
    T = np.stack(cols, axis=1)
    assert T.shape[1] == len(profiled)

    order, root = _reverse_level_order(pb), MR.root_of(pb)
    names = _node_names(pb, species, order)
    head, fields, rows = _read(os.path.join(str(tmp_path), model + "_rate_shift_scan.tab"))
    assert "%d families" % pb.n_families in head
    want_fields = ["Node"] + ["Branch" + c for c in COLUMNS] + ["Clade" + c for c in COLUMNS] + (["BirthDeathT", "BirthDeathP"] if n_par == 2 else []) + ["Note"]
    assert fields == want_fields
    nodes = [v for v in order if v != root]
    assert [r[0] for r in rows] == [names[v] for v in nodes]
    dirs = BR.directions(pb, n_par, Pdim)
    tests = {kind: [BR.score_test(U, G, dirs[v][i], T) for v in nodes] for i, kind in enumerate(("Branch", "Clade"))}
    worst = 0.0
    for kind in ("Branch", "Clade"):
        holm = BR.holm([t["p"] for t in tests[kind]])
        for row, v, t, h in zip(rows, nodes, tests[kind], holm):
            cell = dict(zip(fields, row))
            note = "%s not testable" % kind.lower()
            assert (note in cell["Note"]) == (not t["testable"]), (kind, v, cell["Note"], t)
            vals = [float(cell[kind + c]) for c in COLUMNS]
            if not t["testable"]:
                assert all(np.isnan(x) for x in vals), (kind, v)
                continue
            a = dirs[v][0 if kind == "Branch" else 1]
            gaa = float(a @ G @ a)
            want = [t["U"][0], t["V"][0, 0], t["stat"], t["p"], h, t["multiplier"]]
            floors = [1e-8 * np.sqrt(gaa), 1e-12 * gaa, 1e-12, 0.0, 0.0, 0.0]
            for c, x, w, fl in zip(COLUMNS, vals, want, floors):
                worst = max(worst, abs(x - w) / (1e-8 * abs(w) + fl + 1e-300))
                assert _close(x, w, fl), (kind, v, c, x, w)
    if n_par == 2:
        nonroot = [v for v in range(pb.n_nodes) if v != root]
        for row, v in zip(rows, nodes):
            cell = dict(zip(fields, row))
            A = np.zeros((Pdim, 2))
            A[nonroot.index(v), 0] = A[nb + nonroot.index(v), 1] = 1.0
            t = BR.score_test(U, G, A, T)
            assert ("birth-death not testable" in cell["Note"]) == (not t["testable"]), v
            if t["testable"]:
                assert _close(float(cell["BirthDeathT"]), t["stat"], 1e-12) and _close(float(cell["BirthDeathP"]), t["p"]), v
    print("%s %s: worst |table - numpy| / tolerance %.3g" % (model, extra, worst))
    if "-y" in extra:                                        # the clade of all lambda-2 branches is lambda 2's own direction
        two = [v for v in nodes if pb.lambda_index[v] == 1]
        top = [v for v in two if pb.parent[v] not in two]
        assert len(top) == 1 and sorted(BR.subtree(pb, top[0])) == sorted(two)
        assert not tests["Clade"][nodes.index(top[0])]["testable"] and tests["Branch"][nodes.index(top[0])]["testable"]

    # the lambda tree: written exactly when the smallest Holm-adjusted clade p is below the threshold
    holm = BR.holm([t["p"] for t in tests["Clade"]])
    best = int(np.nanargmin(holm))
    assert _close(info["smallest_clade_holm_p"], holm[best])
    path = os.path.join(str(tmp_path), model + "_rate_shift_lambda_tree.txt")
    assert info["lambda_tree_written"] == (holm[best] < info["threshold"]) == os.path.exists(path)
    if not info["lambda_tree_written"]:
        assert "no rate shift passed the threshold" in r.stderr
        return
    candidates = [nodes[i] for i in range(len(nodes)) if holm[i] == holm[best]]
    tree = P.parse_newick(open(path).read(), lambda_tree=True)
    labelled = {n.key() for n in tree.postorder() if n.lambda_index == 2}
    keys = {v: "".join(sorted(species[pb.leaf_taxon[x]] for x in BR.subtree(pb, v) if pb.leaf_taxon[x] >= 0)) for v in range(pb.n_nodes)}
    assert any(labelled == {keys[x] for x in BR.subtree(pb, v)} for v in candidates), labelled
    assert {n.lambda_index for n in tree.postorder()} == {1, 2}
    assert [n.key() for n in tree.postorder()] == [n.key() for n in P.parse_newick(read("synth20_tree.txt")).postorder()]
