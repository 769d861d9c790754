"""cafe_branch_change's model, on the CPU: the numpy reference of tests/branch_change_ref.py (the branch joint formed explicitly,
its diagonals summed) against a brute-force enumeration of every interior assignment on trees of four taxa with M <= 6 -- every
output to 1e-12 -- its identities with tests/marginal_ref.py, and what the tables of tests/test_branch_change_gpu.py can tell:
four deliberately wrong passes each move some output by more than 1e-6 there, four orders above the GPU test's tolerance.  Also:
the library exports the entry, the header declares it, the ABI version is unchanged, and the driver's refusals hold."""
import functools
import os
import subprocess

import numpy as np
import pytest

import branch_change_ref as BR
import marginal_ref as MR
from cafexp_amd import problem as P
from oracle import oracle as O
from test_marginal_model import _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
TOL = 1e-12


def _tiny():
    out = {}
    pb = _problem("((A:1,B:2):3,(C:1,D:1):2);", [dict(A=1, B=2, C=3, D=1), dict(A=0, B=0, C=2, D=1), dict(A=6, B=5, C=6, D=4)], 6, 5)
    out["binary4"] = (pb, P.Params(lambdas=np.array([0.08]), prior=P.prior_uniform(5)))
    # a polytomy, a leaf under the root, R > M
    pb = _problem("((A:2,B:2,C:1):3,D:5);", [dict(A=1, B=2, C=3, D=1), dict(A=0, B=0, C=0, D=2)], 5, 6)
    out["polytomy_root_above"] = (pb, P.Params(lambdas=np.array([0.06]), prior=P.prior_poisson(6, 2.0)))
    pb = _problem("((A:1,B:2):3,(C:1,D:1):2);", [dict(A=1, B=2, C=3, D=1), dict(A=5, B=0, C=1, D=2)], 6, 4, lambda_tree="((A:1,B:1):1,(C:2,D:2):2);")
    out["two_lambdas"] = (pb, P.Params(lambdas=np.array([0.03, 0.12]), prior=P.prior_uniform(4)))
    pb = _problem("((A:1,B:2):3,(C:2,D:1):1);", [dict(A=1, B=2, C=3, D=0), dict(A=0, B=1, C=0, D=0), dict(A=6, B=5, C=6, D=6)], 6, 4, n_dev=3)
    pr = P.Params(lambdas=np.array([0.07]), prior=P.prior_uniform(4))
    pr.error_model = P.error_model_table(P.default_error_model(6), 6)
    out["error_model"] = (pb, pr)
    pb = _problem("((A:1,B:2):3,(C:1,D:1):2);", [dict(A=1, B=2, C=3, D=1), dict(A=3, B=0, C=1, D=0)], 6, 5)
    pr = P.Params(lambdas=np.array([0.06]), prior=P.prior_uniform(5))
    pr.cat_probs, pr.multipliers = O.discrete_gamma(2, 0.7)
    out["gamma2"] = (pb, pr)
    return out


TINY = _tiny()


def _close(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    s = np.abs(b) if scale is None else np.asarray(scale, dtype=np.float64)
    assert np.all(np.abs(a[ok] - b[ok]) <= TOL * s[ok]), (a, b)


@pytest.mark.parametrize("name", sorted(TINY))
def test_the_reference_equals_brute_force(name):
    pb, pr = TINY[name]
    assert pb.max_family_size <= 6 and len(pb.taxa) == 4
    mats = MR.oracle_matrices(pb, pr, O)
    top = max(pb.max_family_size, pb.max_root_family_size)
    for f in range(pb.n_families):
        state = BR.diagonals_family(pb, pr, mats, f)
        for D, level in ((0, 0.95), (1, 0.5), (2, 0.95), (top, 0.8)):
            ref = BR.summarise_family(pb, state, D, level)
            bf = BR.brute_force_family(pb, pr, mats, f, D, level)
            assert ref["failed"] == bf["failed"] == 0
            for key in ("pmf", "below", "above"):
                _close(ref[key], bf[key])
            _close(ref["mean"], bf["mean"], scale=bf["mean_scale"])
            _close(ref["log_evidence"], bf["log_evidence"])
            for key in ("mode", "lo", "hi"):
                tie = bf[key + "_gap"] <= 1e-12          # integers are exact unless the enumeration itself sits on a tie
                assert np.array_equal(ref[key][~tie], bf[key][~tie]), (key, D, ref[key], bf[key])
            if D == top:
                assert np.all(ref["below"][~np.isnan(ref["below"])] == 0.0) and np.all(ref["above"][~np.isnan(ref["above"])] == 0.0)


@pytest.mark.parametrize("name", sorted(TINY))
def test_identities_with_the_marginal_reconstruction(name):
    """sum pmf + below + above = 1; the mass above 0 is marginal_ref's p_increase, the mass below 0 its p_decrease; mean is the
    difference of the two nodes' posterior means; the root is NaN and CAFE_CHANGE_NONE."""
    pb, pr = TINY[name]
    mats = MR.oracle_matrices(pb, pr, O)
    root = MR.root_of(pb)
    mr = MR.updown(pb, pr, mats, 0.95, detail=True)
    sizes = np.arange(mr["post"].shape[2])
    node_mean = (mr["post"] * sizes).sum(axis=2) / mr["Z"][:, None]
    for D in (0, 1, 3):
        ref = BR.change(pb, pr, mats, D, 0.95)
        inner = np.array([v for v in range(pb.n_nodes) if v != root])
        total = ref["pmf"][:, inner].sum(axis=2) + ref["below"][:, inner] + ref["above"][:, inner]
        assert np.all(np.abs(total - 1.0) <= TOL)
        up = ref["pmf"][:, inner, D + 1:].sum(axis=2) + ref["above"][:, inner]
        down = ref["pmf"][:, inner, :D].sum(axis=2) + ref["below"][:, inner]
        assert np.all(np.abs(up - mr["p_increase"][:, inner]) <= TOL) and np.all(np.abs(down - mr["p_decrease"][:, inner]) <= TOL)
        want = node_mean[:, inner] - node_mean[:, pb.parent[inner]]
        assert np.all(np.abs(ref["mean"][:, inner] - want) <= TOL * ref["mean_scale"][:, inner])
        assert np.all(np.isnan(ref["pmf"][:, root])) and np.all(np.isnan(ref["mean"][:, root])) and np.all(np.isnan(ref["below"][:, root]))
        for key in ("mode", "lo", "hi"):
            assert np.all(ref[key][:, root] == BR.NONE) and np.all(ref[key][:, inner] != BR.NONE)
            assert np.all(np.abs(ref[key][:, inner]) <= D + 1)
    np.testing.assert_allclose(BR.change(pb, pr, mats, 1, 0.95)["log_evidence"], mr["log_evidence"], rtol=TOL)


def test_a_failed_family_is_nan_and_none():
    pb, pr = TINY["binary4"]
    pr = P.Params(lambdas=np.array([5.0]), prior=pr.prior)           # saturated: every row s >= 1 of every matrix is 0
    ref = BR.change_family(pb, pr, MR.oracle_matrices(pb, pr, O), 0, 2, 0.95)
    assert ref["failed"] == 1 and np.isnan(ref["log_evidence"])
    for key in ("pmf", "below", "above", "mean"):
        assert np.all(np.isnan(ref[key])), key
    for key in ("mode", "lo", "hi"):
        assert np.all(ref[key] == BR.NONE), key


# ------------------------------------------------------------------------------- what the GPU test's tables can tell
MUTANT_D = 3


@functools.lru_cache(maxsize=None)
def _gpu_table_case(order, model):
    pb = BR.problem(order, model)
    pr = BR.params(pb, model)
    mats = MR.oracle_matrices(pb, pr, O)
    return pb, pr, mats, BR.summarise(pb, BR.diagonals(pb, pr, mats), MUTANT_D, 0.95)


@pytest.mark.parametrize("order,model", [(41, "base"), (41, "error3"), (41, "error5"), (300, "base"), (300, "error3")])
def test_the_gpu_tables_tell_a_wrong_pass_from_a_right_one(order, model):
    """On the very tables of test_branch_change_gpu.py (oracle matrices): d taken as i - j, the i = 0 row dropped, the tail mask >=
    for >, and -- under an error model -- the tap offset ignored each move a probability or a mean by more than 1e-6."""
    pb, pr, mats, ref = _gpu_table_case(order, model)
    assert not ref["failed"].any()
    for mutant in BR.MUTANTS:
        if mutant == "tap_offset_ignored" and pr.error_model is None:
            continue
        mut = BR.summarise(pb, BR.diagonals(pb, pr, mats, mutant=mutant), MUTANT_D, 0.95, mutant=mutant)
        shift = BR.max_shift(mut, ref)
        print("order %d %s %s: largest shift %.3g" % (order, model, mutant, shift))
        assert shift > 1e-6, (order, model, mutant, shift)


@pytest.mark.parametrize("order", [41, 300])
def test_the_row_0_term_is_material_where_a_whole_clade_is_at_zero(order):
    """G[0] B[0] -- the parent and the node both extinct -- is the term the band kernel adds outside its loop.  The families whose
    clade ((A,B),G) is all zero put posterior mass on it at the branches inside that clade: dropping the row moves their pmf[0]
    by more than 1e-6; a family with a positive count in every clade is not moved at all."""
    pb, pr, mats, ref = _gpu_table_case(order, "base")
    col = {s: pb.taxa.index(s) for s in "ABG"}
    clade_zero = np.where((pb.counts[:, [col["A"], col["B"], col["G"]]] == 0).all(axis=1))[0]
    positive = np.where((pb.counts > 0).all(axis=1))[0][:20]
    assert len(clade_zero) >= 6 and len(positive) >= 10          # the all-zero family, its repeat, and branch_change_ref.CLADE_AT_ZERO
    mut = BR.summarise(pb, BR.diagonals(pb, pr, mats, families=clade_zero, mutant="row0_dropped"), MUTANT_D, 0.95)
    inner = [v for v in range(pb.n_nodes) if pb.leaf_taxon[v] < 0 and v != MR.root_of(pb)]      # the band kernel's branches
    d = np.abs(mut["pmf"][:, inner, MUTANT_D] - ref["pmf"][clade_zero][:, inner, MUTANT_D])
    print("order %d: row 0 carries up to %.3g of a branch's posterior over %d families" % (order, float(np.nanmax(d)), len(clade_zero)))
    assert np.all(np.nanmax(d, axis=1) > 1e-6)
    same = BR.summarise(pb, BR.diagonals(pb, pr, mats, families=positive, mutant="row0_dropped"), MUTANT_D, 0.95)
    assert BR.max_shift(same, {k: ref[k][positive] for k in ("pmf", "below", "above", "mean")}) <= 1e-15


def test_the_tables_are_what_the_gpu_test_needs():
    pb = BR.problem(41)
    assert len(pb.taxa) == 7 and pb.n_families <= 400
    distinct = len(np.unique(pb.counts, axis=0))
    assert 2 * 128 < distinct < 3 * 128 and pb.n_families > distinct       # three column tiles, the last partial; repeated rows
    ch, root = MR.children_of(pb), MR.root_of(pb)
    assert any(len(ch[v]) >= 3 for v in range(pb.n_nodes))                  # a polytomy
    assert any(pb.leaf_taxon[v] >= 0 for v in ch[root])                     # a leaf under the root
    assert any(pb.leaf_taxon[v] < 0 for v in ch[root])                      # an interior branch under the root: np = R
    assert any(pb.leaf_taxon[v] < 0 and v != root and pb.parent[v] != root for v in range(pb.n_nodes))     # and one below: np = M
    assert (BR.problem(300).max_family_size, BR.problem(300).max_root_family_size) == (299, 250)
    rb = BR.root_above_problem()
    assert rb.max_root_family_size > rb.max_family_size


# ------------------------------------------------------------------------------- exports and refusals
def test_the_library_exports_the_entry_and_the_abi_version_stays():
    from cafexp_amd import capi
    assert "cafe_branch_change" in capi.EXPORTS
    lib = capi.load()
    assert getattr(lib, "cafe_branch_change") is not None
    assert lib.cafe_abi_version() == 3
    assert hasattr(capi.Context, "branch_change")
    assert capi.CAFE_CHANGE_NONE == BR.NONE == -2147483648
    with open(os.path.join(ROOT, "include", "cafe_mi355x.h")) as f:
        header = f.read()
    assert "int cafe_branch_change(cafe_ctx* ctx, const cafe_params* params, int32_t max_change, double level, const cafe_branch_change_out* out);" in header
    assert "#define CAFE_ABI_VERSION 3" in header and "#define CAFE_CHANGE_NONE" in header


def test_the_driver_names_the_flag_and_refuses_what_it_cannot_do():
    assert os.path.exists(EXE), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 2 and "--branch-change" in r.stderr
    data = os.path.join(ROOT, "tests", "golden", "data")
    base = [EXE, "-t", os.path.join(data, "mammals_tree.txt"), "-i", os.path.join(data, "mammal_gene_families.txt"), "-l", "0.0018", "--branch-change"]
    for extra, word in ((["--missing", "NA"], "missing cells"), (["--mask-cells", "cells.txt"], "missing cells"), (["--gpus", "2"], "--gpus"),
                        (["-b"], "-b"), (["-3"], None), (["5", "-P", "1.5"], "PVALUE")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        if word is None:
            assert r.returncode == 2, extra                       # "-3" is no D: an unknown option
            continue
        assert r.returncode == 1 and "--branch-change" in r.stderr and word in r.stderr, (extra, r.stderr)
    r = subprocess.run([EXE, "-t", os.path.join(data, "mammals_tree.txt"), "-l", "0.0018", "--simulate", "5", "--branch-change"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--branch-change" in r.stderr and "--simulate" in r.stderr
