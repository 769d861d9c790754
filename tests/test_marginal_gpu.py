"""cafe_marginal_reconstruct on the device against tests/marginal_ref.py fed the matrices the call itself built
(Context.matrix), so that K1's pinned parity is not tested again.

Doubles: |d| <= 1e-12 + 1e-10 |ref| -- every sum is over at most 2048 non-negative terms, so the error is of order
N eps = 2e-13 per GEMM without cancellation; 1e-10 is the project's bound for the scorer against the oracle.
Integers (mode, lo, hi): exact, except where the reference's own CDF lies within 1e-9 of the threshold or its two best masses
within 1e-9 relative; such cells are at most 1 % of a case's cells (the reference alone reports less: asserted)."""
import json
import os
import subprocess

import numpy as np
import pytest

import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import case_from_args, read, table
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAMMALS = {"tree": "mammals_tree.txt", "families": "mammal_gene_families.txt"}
# synth20's species under a tree with a trifurcating root and two polytomies below it
SYNTH20_NONBINARY = ("((t015:11.275,t006:11.276,t013:11.276):88.725,(t011:22.883,t016:22.883,(t001:2.202,t014:2.202):20.68):77.117,"
                     "((t010:17.606,t000:17.606,t019:17.606):20.132,((t012:0.948,t017:0.948):20.533,(t003:18.062,t007:18.062,t008:18.062):3.419):16.258,"
                     "((t004:8.036,t018:8.036):27.359,(t002:27.874,(t005:26.756,t009:26.756):1.118):7.521):2.343):62.261);")

CASES = {
    "mammals_one_lambda": dict(MAMMALS, limit=32, **{"lambda": 0.0018}),
    "mammals_two_lambdas": dict(MAMMALS, limit=24, lambdas="0.01,0.05", lambda_tree="chimphuman_separate_lambda.txt"),
    "mammals_error_model": dict(MAMMALS, limit=24, errfile="errormodel_0.1.txt", **{"lambda": 0.0018}),
    "mammals_poisson": dict(MAMMALS, limit=24, prior="poisson:10", **{"lambda": 0.01}),
    "mammals_gamma_k3": dict(MAMMALS, limit=24, model="gamma", k=3, alpha=0.425, **{"lambda": 0.002}),
    "large6_order_1126": dict(tree="large6_tree.txt", families="large6_families.txt", limit=3, **{"lambda": 0.001}),
}


def _case(name):
    if name == "synth20_nonbinary":
        species, ids, counts = table("synth20_families.txt")
        pb = P.build_problem(P.parse_newick(SYNTH20_NONBINARY), species, ids, counts)
        pb.counts = np.ascontiguousarray(pb.counts[:24])
        pb.family_ids = pb.family_ids[:24]
        return pb, P.Params(lambdas=np.array([0.004]), prior=P.prior_uniform(pb.max_root_family_size)), 1.0
    return case_from_args(CASES[name], O)


def _K(pr):
    return 1 if pr.multipliers is None else len(pr.multipliers)


def _compare(got, ref, label):
    """Prints every figure before it asserts; returns the share of excused integer cells."""
    worst = {}
    for key in ("mean", "p_increase", "p_decrease", "log_evidence"):
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key)
        ok = ~np.isnan(r)
        excess = np.abs(g[ok] - r[ok]) - (1e-12 + 1e-10 * np.abs(r[ok]))
        worst[key] = float(np.max(np.abs(g[ok] - r[ok]) / (1e-12 + 1e-10 * np.abs(r[ok])))) if ok.any() else 0.0
        print("%s %s: worst |d| / bound = %.3g" % (label, key, worst[key]))
        assert np.all(excess <= 0), (label, key, worst[key])
    assert np.array_equal(got["failed"], ref["failed"]), label
    n_exc, n_cells = 0, 0
    for key, mask in zip(("mode", "lo", "hi"), MR.excused(ref)):
        diff = np.asarray(got[key]) != np.asarray(ref[key])
        print("%s %s: %d differ, %d excusable of %d" % (label, key, int(diff.sum()), int(mask.sum()), diff.size))
        assert not np.any(diff & ~mask), (label, key, np.argwhere(diff & ~mask)[:5])
        n_exc += int(mask.sum())
        n_cells += diff.size
    share = n_exc / n_cells
    print("%s: excusable share %.4f" % (label, share))
    assert share < 0.01, (label, share)                      # the reference alone stays below 1 %
    return share


def _invariants(got):
    ok = got["failed"] == 0
    assert np.all(got["lo"][ok] <= got["mode"][ok]) and np.all(got["mode"][ok] <= got["hi"][ok])
    s = (got["p_increase"] + got["p_decrease"])[ok]
    s = s[~np.isnan(s)]
    assert np.all(s >= 0) and np.all(s <= 1 + 1e-12)


@pytest.mark.parametrize("name", sorted(CASES) + ["synth20_nonbinary"])
def test_matches_the_numpy_updown_pass(name):
    from cafexp_amd import capi
    pb, pr, alpha = _case(name)
    K = _K(pr)
    ctx = capi.Context(pb, max_categories=K)
    for level in (0.95, 0.5):
        got = ctx.marginal_reconstruct(pr, level=level, alpha=alpha)
        mats = MR.context_matrices(ctx, pb, K)
        ref = MR.updown(pb, pr, mats, level)
        _compare(got, ref, "%s level %.2f" % (name, level))
        _invariants(got)
    root = MR.root_of(pb)
    assert np.all(np.isnan(got["p_increase"][:, root])) and np.all(np.isnan(got["p_decrease"][:, root]))
    if pr.error_model is None:
        leaves = np.where(pb.leaf_taxon >= 0)[0]
        for key in ("mode", "lo", "hi"):
            assert np.array_equal(got[key][:, leaves], pb.counts[:, pb.leaf_taxon[leaves]])
    ctx.close()


@pytest.mark.parametrize("name", ["mammals_one_lambda", "mammals_poisson", "mammals_gamma_k3", "mammals_error_model"])
def test_tie_to_the_shipped_scorer(name):
    """After ctx.score, root_likelihoods(f) * prior, normalised (and mixed over the categories), gives the same root mean and
    log evidence; and log_evidence >= family_lnl (the scorer takes the largest term of the sum)."""
    from cafexp_amd import capi
    pb, pr, alpha = _case(name)
    K = _K(pr)
    ctx = capi.Context(pb, max_categories=K)
    got = ctx.marginal_reconstruct(pr, alpha=alpha)
    _, fam = ctx.score(pr, alpha=alpha, per_family=True)
    probs = [1.0] if pr.cat_probs is None else pr.cat_probs
    prior = np.asarray(pr.prior, dtype=np.float32).astype(np.float64)
    root = MR.root_of(pb)
    sizes = np.arange(1, pb.max_root_family_size + 1)
    for f in range(pb.n_families):
        post = sum(probs[k] * ctx.root_likelihoods(f, k) * prior for k in range(K))
        z = post.sum()
        for g, r in ((got["log_evidence"][f], np.log(z)), (got["mean"][f, root], (sizes * post).sum() / z)):
            assert abs(g - r) <= 1e-12 + 1e-10 * abs(r), (name, f, g, r)
        assert got["log_evidence"][f] >= fam["family_lnl"][f] - 1e-12
    ctx.close()


def test_failed_family_keeps_the_call_ok():
    """A saturating lambda gives every family zero likelihood: failed = 1, NaN doubles, -1 integers, the call returns OK."""
    from cafexp_amd import capi
    pb, pr, _ = _case("mammals_one_lambda")
    ctx = capi.Context(pb)
    bad = P.Params(lambdas=np.array([0.5]), prior=pr.prior)
    got = ctx.marginal_reconstruct(bad)
    assert np.all(got["failed"] == 1)
    for key in ("mean", "p_increase", "p_decrease", "log_evidence"):
        assert np.all(np.isnan(got[key])), key
    for key in ("mode", "lo", "hi"):
        assert np.all(got[key] == -1), key
    good = ctx.marginal_reconstruct(pr)
    assert np.all(good["failed"] == 0)
    ctx.close()


def test_argument_and_state_errors():
    from cafexp_amd import capi
    pb, pr, _ = _case("mammals_one_lambda")
    ctx = capi.Context(pb)
    for level in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.marginal_reconstruct(pr, level=level)
    with pytest.raises(capi.CafeError, match="code 1"):
        ctx.marginal_reconstruct(P.Params(lambdas=np.array([-0.01]), prior=pr.prior))
    gpr = P.Params(lambdas=pr.lambdas, prior=pr.prior)
    gpr.cat_probs, gpr.multipliers = O.discrete_gamma(3, 0.5)
    with pytest.raises(capi.CafeError, match="code 1"):      # the context was made for one category
        ctx.marginal_reconstruct(gpr)
    ctx.close()


def test_batches_and_duplicates_change_no_bit():
    """Duplicated families with dedup on and off, and a workspace_limit small enough for several column batches: the same
    bits as one batch over the distinct families."""
    from cafexp_amd import capi
    pb, pr, _ = _case("mammals_one_lambda")
    reps = np.concatenate([np.arange(pb.n_families)] * 9 + [np.arange(5)])      # 293 families: three 128-column tiles without dedup
    big = P.Problem(parent=pb.parent, branch_length=pb.branch_length, lambda_index=pb.lambda_index, leaf_taxon=pb.leaf_taxon,
                    counts=np.ascontiguousarray(pb.counts[reps]), max_family_size=pb.max_family_size,
                    max_root_family_size=pb.max_root_family_size, taxa=pb.taxa, family_ids=["d%d" % i for i in range(len(reps))],
                    node_names=pb.node_names)
    base = capi.Context(pb)
    want = base.marginal_reconstruct(pr)
    base.close()
    nI = int((pb.leaf_taxon < 0).sum())
    per_col = (4 * nI + 2) * pb.matrix_size * 8 + 4096       # panels of one column, with room for the small arrays
    for dedup, limit in ((True, 0), (False, 0), (False, 130 * per_col)):
        ctx = capi.Context(big, dedup=dedup, workspace_limit=limit)
        got = ctx.marginal_reconstruct(pr)
        for key in want:
            assert np.array_equal(got[key], want[key][reps], equal_nan=True), (dedup, limit, key)
        ctx.close()


def test_no_side_effect_on_the_scorer():
    from cafexp_amd import capi
    pb, pr, alpha = _case("mammals_gamma_k3")
    ctx = capi.Context(pb, max_categories=3)
    before, fam0 = ctx.score(pr, alpha=alpha, per_family=True)
    ctx.marginal_reconstruct(pr, alpha=alpha)
    after, fam1 = ctx.score(pr, alpha=alpha, per_family=True)
    assert np.float64(before).tobytes() == np.float64(after).tobytes()
    for key in fam0:
        assert np.array_equal(fam0[key], fam1[key]), key
    ctx.close()


def _reverse_level_order(pb):
    ch, order, q = MR.children_of(pb), [], [MR.root_of(pb)]
    while q:
        v = q.pop(0)
        order.append(v)
        q.extend(ch[v])
    return order[::-1]


def _read_tab(path):
    with open(path) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    return rows[0], rows[1:]


@pytest.mark.parametrize("model", ["Base", "Gamma"])
def test_driver_writes_the_posterior_tables(tmp_path, model):
    from cafexp_amd import capi
    exe = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
    assert os.path.exists(exe), "cafexp_hip missing: run __graft_entry__.build()"
    data = os.path.join(ROOT, "tests", "golden", "data")
    args = dict(MAMMALS, limit=40, **{"lambda": 0.0018})
    cmd = [exe, "-t", os.path.join(data, args["tree"]), "-i", os.path.join(data, args["families"]), "-l", "0.0018", "--limit", "40",
           "--reconstruct", "--reconstruct-marginal", "0.9", "-o", str(tmp_path)]
    if model == "Gamma":
        args.update(model="gamma", k=3, alpha=0.7)
        cmd += ["-k", "3", "-a", "0.7"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    js = json.loads(out.stdout.strip().splitlines()[-1])
    assert js["marginal"]["level"] == 0.9 and js["marginal"]["failed"] == 0 and js["marginal"]["seconds"] >= 0
    pb, pr, alpha = case_from_args(args, O)
    assert js["n_families"] == pb.n_families
    ctx = capi.Context(pb, max_categories=_K(pr))
    got = ctx.marginal_reconstruct(pr, level=0.9, alpha=alpha)
    ctx.close()
    head_s, rows_s = _read_tab(os.path.join(str(tmp_path), model + "_posterior_sizes.tab"))
    head_c, rows_c = _read_tab(os.path.join(str(tmp_path), model + "_posterior_change.tab"))
    head_n, rows_n = _read_tab(os.path.join(str(tmp_path), model + "_count.tab"))
    assert head_s == head_n and head_c == head_n
    assert [r[0] for r in rows_s] == [r[0] for r in rows_n] == [r[0] for r in rows_c] == list(pb.family_ids)
    order = _reverse_level_order(pb)
    root = MR.root_of(pb)
    for f in range(pb.n_families):
        for col, v in enumerate(order):
            mean, mode, iv = rows_s[f][1 + col].split(":")
            lo, hi = iv.split("-")
            assert mean == "%.6g" % got["mean"][f, v]
            assert (int(mode), int(lo), int(hi)) == (got["mode"][f, v], got["lo"][f, v], got["hi"][f, v])
            cell = rows_c[f][1 + col]
            if v == root:
                assert cell == "-"
            else:
                assert cell == "%.6g:%.6g" % (got["p_decrease"][f, v], got["p_increase"][f, v])


def test_driver_refuses_several_gpus(tmp_path):
    exe = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
    data = os.path.join(ROOT, "tests", "golden", "data")
    out = subprocess.run([exe, "-t", os.path.join(data, "mammals_tree.txt"), "-i", os.path.join(data, "mammal_gene_families.txt"), "-l", "0.0018",
                          "--gpus", "2", "--reconstruct-marginal"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "--gpus" in out.stderr
