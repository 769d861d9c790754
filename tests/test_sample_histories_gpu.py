"""cafe_sample_histories on the device, replayed draw for draw by tests/history_ref.py fed the matrices the call itself
built (marginal_ref.context_matrices): every history that the helper does not flag ambiguous (a target within the rounding
band of a prefix-sum entry, history_ref's docstring) is EQUAL in sizes and category, and at most 1e-3 of a case's histories
are left out.  Then invariants, determinism, the library's own marginals, failures, arguments and the driver."""
import contextlib
import faulthandler
import json
import os
import re
import subprocess

import numpy as np
import pytest

import history_ref as HR
import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import case_from_args
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
LEFT_OUT = 1e-3
KEYS = ("category", "n_increase", "n_decrease", "net_change", "log_evidence", "failed")
STEP_SECONDS = 120


@contextlib.contextmanager
def _limit(seconds=STEP_SECONDS):
    """The time limit of one step that uses the GPU in this process: a step that hangs ends the process with every thread's
    stack printed (the watchdog is a thread of its own, so it fires while the step blocks inside the library); a step that
    returns waits for nothing."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _context(case, **kw):
    from cafexp_amd import capi
    with _limit():
        ctx = capi.Context(case["pb"], max_categories=case["K"], **kw)
        if case["mus"] is not None:
            ctx.set_death_rates(case["mus"])
    return ctx


def _draw(ctx, case, **kw):
    with _limit():
        return ctx.sample_histories(case["pr"], case["n_draws"], case["seed"], alpha=case["alpha"], **kw)


def _same(a, b, keys):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def _invariants(pb, pr, got):
    sizes = got["sizes"]
    M, R, root = pb.max_family_size, pb.max_root_family_size, MR.root_of(pb)
    assert sizes.min() >= 0 and sizes.max() <= max(M, R)
    assert sizes[:, :, root].min() >= 1 and sizes[:, :, root].max() <= R
    others = [v for v in range(pb.n_nodes) if v != root]
    assert sizes[:, :, others].max() <= M
    for v in others:
        assert not sizes[:, :, v][sizes[:, :, pb.parent[v]] == 0].any(), v      # a child of a 0 parent is 0
    if pr.error_model is None:
        leaves = np.where(pb.leaf_taxon >= 0)[0]
        assert np.array_equal(sizes[:, :, leaves], np.broadcast_to(pb.counts[:, pb.leaf_taxon[leaves]], sizes[:, :, leaves].shape))
    for key, val in HR.recount(pb, sizes).items():
        assert np.array_equal(got[key], val), key
    assert got["net_change"][:, root].tolist() == [0] * sizes.shape[0]


@pytest.mark.parametrize("name", sorted(HR.CASES))
def test_replayed_draw_for_draw(name):
    case = HR.CASES[name]()
    pb, pr = case["pb"], case["pr"]
    ctx = _context(case)
    got = _draw(ctx, case)
    with _limit():
        mats = MR.context_matrices(ctx, pb, case["K"])
    ref = HR.sample(pb, pr, mats, case["n_draws"], case["seed"])
    lean = _draw(ctx, case, sizes=False)
    ctx.close()
    keep = ~ref["ambiguous"].T                               # [draw][family]
    print("%s: %d histories compared, %d left out" % (name, keep.sum(), (~keep).sum()))
    assert (~keep).mean() <= LEFT_OUT
    assert np.array_equal(got["failed"], ref["failed"]) and not got["failed"].any()
    assert np.allclose(got["log_evidence"], ref["log_evidence"], rtol=1e-10, atol=1e-12)
    bad = np.argwhere(keep & ((got["sizes"] != ref["sizes"]).any(axis=2) | (got["category"] != ref["category"])))
    assert len(bad) == 0, "%s: %d histories differ, first (draw, family) %s: device %s category %d, replay %s category %d" % (
        name, len(bad), bad[0], got["sizes"][tuple(bad[0])], got["category"][tuple(bad[0])], ref["sizes"][tuple(bad[0])], ref["category"][tuple(bad[0])])
    _invariants(pb, pr, got)
    assert "sizes" not in lean
    _same(got, lean, KEYS)
    if case["K"] > 1:
        assert len(np.unique(got["category"])) > 1


def _mammals(**extra):
    return case_from_args(dict(tree="mammals_tree.txt", families="mammal_gene_families.txt", limit=64, **extra), O)


def test_same_bits_twice_in_batches_and_across_duplicates():
    case = HR._case(HR.CATERPILLAR, 24, 20, 90, 100, 33, 22, gamma=3)      # 7 interior nodes: 130 columns of panels also hold cafe_create's own
    pb, pr = case["pb"], case["pr"]
    reps = np.repeat(np.arange(pb.n_families), 4)            # every family 4 times: 400 families over 90 columns ...
    big = P.Problem(parent=pb.parent, branch_length=pb.branch_length, lambda_index=pb.lambda_index, leaf_taxon=pb.leaf_taxon,
                    counts=np.ascontiguousarray(pb.counts[reps]), max_family_size=pb.max_family_size, max_root_family_size=pb.max_root_family_size,
                    taxa=pb.taxa, family_ids=["d%d" % i for i in range(len(reps))], node_names=pb.node_names)
    wide = dict(case, pb=big)
    ctx = _context(wide, dedup=False)                        # ... and without dedup 400 columns: four 128-column tiles
    a, b = _draw(ctx, wide), _draw(ctx, wide)
    ctx.close()
    _same(a, b, KEYS + ("sizes",))
    nI = int((pb.leaf_taxon < 0).sum())
    # A limit sized after history.hip's rule (the counts of all draws first, then three quarters of the rest for B and F of
    # every interior node, Z_k and Z of a column batch) to hold between one and two 128-column tiles.  What it forced is
    # read back and asserted, so a changed rule fails here instead of leaving one batch and one pass.
    per_col = (2 * nI * pb.matrix_size + case["K"] + 1) * 8
    limit = (190 * per_col * 4) // 3 + 3 * case["n_draws"] * pb.n_nodes * 8
    ctx = _context(wide, dedup=False, workspace_limit=limit)
    c = _draw(ctx, wide)
    batches, passes = ctx.history_batches()
    ctx.close()
    print("workspace_limit %d: %d column batches, %d draw passes each" % (limit, batches, passes))
    assert batches >= 3 and big.n_families % 128 != 0 and passes > 1           # (the last batch is a partial tile)
    _same(a, c, KEYS + ("sizes",))
    ctx = _context(wide)                                     # dedup on: 90 columns shared by 4 families each
    d = _draw(ctx, wide)
    ctx.close()
    _same(a, d, KEYS + ("sizes",))
    for f in range(0, big.n_families, 4):
        assert len(set(d["log_evidence"][f:f + 4].tobytes()[i:i + 8] for i in range(0, 32, 8))) == 1
    spread = a["sizes"].reshape(case["n_draws"], pb.n_families, 4, pb.n_nodes)
    distinct = [len({spread[:, f, r].tobytes() for r in range(4)}) for f in range(pb.n_families)]
    interior = np.where(pb.leaf_taxon < 0)[0]
    loose = [f for f in range(pb.n_families) if len(np.unique(spread[:, f, 0][:, interior], axis=0)) > 1]      # a non-degenerate posterior
    assert len(loose) > pb.n_families // 2 and all(distinct[f] == 4 for f in loose)


@pytest.mark.parametrize("kind", ["base", "gamma_error_model"])
def test_agrees_with_the_marginal_reconstruction(kind):
    """2 000 draws of 64 families against cafe_marginal_reconstruct on the same context: per (family, node) the frequency of
    X_v > X_parent within 6 binomial standard errors of p_increase, the sample mean within 6 standard errors (from the
    sample variance) of mean."""
    from cafexp_amd import capi
    extra = {"lambda": 0.0018} if kind == "base" else dict(model="gamma", k=3, alpha=0.7, errfile="errormodel_0.1.txt", **{"lambda": 0.0018})
    pb, pr, alpha = _mammals(**extra)
    D = 2000
    with _limit():
        ctx = capi.Context(pb, max_categories=1 if pr.multipliers is None else len(pr.multipliers))
        marg = ctx.marginal_reconstruct(pr, alpha=alpha)
        got = ctx.sample_histories(pr, D, 20261018, alpha=alpha)
        ctx.close()
    assert not got["failed"].any() and np.allclose(got["log_evidence"], marg["log_evidence"], rtol=1e-10, atol=1e-12)
    x = got["sizes"].astype(np.float64)                      # [D][F][n]
    root = MR.root_of(pb)
    worst_p = worst_m = 0.0
    for v in range(pb.n_nodes):
        mean, sd = x[:, :, v].mean(axis=0), x[:, :, v].std(axis=0, ddof=1)
        dm = np.abs(mean - marg["mean"][:, v]) / np.maximum(sd / np.sqrt(D), 1e-300)
        dm[np.abs(mean - marg["mean"][:, v]) <= 1e-9] = 0.0  # a node that never varies
        worst_m = max(worst_m, dm.max())
        if v != root:
            p = marg["p_increase"][:, v]
            freq = (x[:, :, v] > x[:, :, pb.parent[v]]).mean(axis=0)
            dp = np.abs(freq - p) / np.maximum(np.sqrt(np.clip(p * (1 - p), 0, None) / D), 1e-300)
            dp[np.abs(freq - p) <= 1e-9] = 0.0
            worst_p = max(worst_p, dp.max())
    print("%s: worst p_increase %.2f and mean %.2f standard errors" % (kind, worst_p, worst_m))
    assert worst_p <= 6 and worst_m <= 6


def test_a_failed_family_leaves_its_neighbours_alone():
    """test_marginal_shapes' construction: A's branch quantizes to t_q = 0, its matrix is e_0 in row 0 and zero below, so a
    family is possible only with A = B = 0.  Half the families are made so, the others fail in the same batch; with the
    failing rows made possible too, the possible families draw the same histories as before."""
    import dataclasses
    from cafexp_amd import capi
    from test_gpu_parity import _random_problem
    pb = _random_problem(np.random.default_rng(5), "((A:0.0004,B:1):1,C:2);", 70, 40, 30, 12)
    counts = pb.counts.copy()
    a, b = pb.taxa.index("A"), pb.taxa.index("B")
    counts[::2, [a, b]] = 0
    pb = dataclasses.replace(pb, counts=counts)
    possible = (counts[:, a] == 0) & (counts[:, b] == 0)
    assert possible.sum() >= 20 and (~possible).sum() >= 20
    pr = P.Params(lambdas=np.array([0.02]), prior=P.prior_uniform(30))
    with _limit():
        ctx = capi.Context(pb)
        got = ctx.sample_histories(pr, 16, 5)
        ctx.close()
    assert np.array_equal(got["failed"] == 0, possible)
    assert np.all(got["sizes"][:, ~possible] == -1) and np.all(got["category"][:, ~possible] == -1) and np.all(np.isnan(got["log_evidence"][~possible]))
    assert np.all(got["sizes"][:, possible] >= 0) and np.all(got["category"][:, possible] == 0) and np.all(np.isfinite(got["log_evidence"][possible]))
    for key, val in HR.recount(pb, got["sizes"]).items():    # (recount leaves the -1 rows out)
        assert np.array_equal(got[key], val), key
    mended = counts.copy()
    mended[:, [a, b]] = 0
    with _limit():
        ctx = capi.Context(dataclasses.replace(pb, counts=mended))
        all_good = ctx.sample_histories(pr, 16, 5)
        ctx.close()
    assert not all_good["failed"].any()
    assert np.array_equal(all_good["sizes"][:, possible], got["sizes"][:, possible])
    assert np.array_equal(all_good["log_evidence"][possible], got["log_evidence"][possible])
    assert (all_good["n_decrease"] >= got["n_decrease"]).all()           # the mended families only add


def test_argument_and_state_errors_and_the_scorer_afterwards():
    from cafexp_amd import capi
    pb, pr, _ = _mammals(**{"lambda": 0.0018})
    with _limit():
        ctx = capi.Context(pb)
        before = ctx.score(pr)
        for n_draws in (0, 65537):
            with pytest.raises(capi.CafeError, match="code 1"):
                ctx.sample_histories(pr, n_draws, 1)
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.sample_histories(P.Params(lambdas=np.array([-0.01]), prior=pr.prior), 4, 1)
        gpr = P.Params(lambdas=pr.lambdas, prior=pr.prior)
        _, gpr.multipliers = O.discrete_gamma(1, 0.5)            # gamma without cat_probs
        with pytest.raises(capi.CafeError, match="code 1"):
            ctx.sample_histories(gpr, 4, 1)
        ctx.sample_histories(pr, 4, 1)
        assert np.float64(ctx.score(pr)).tobytes() == np.float64(before).tobytes()
        ctx.comm_attach(capi.comm_unique_id(), 1, 0)
        with pytest.raises(capi.CafeError, match="code 4"):           # CAFE_ERR_STATE
            ctx.sample_histories(pr, 4, 1)
        ctx.comm_detach()
        ctx.close()


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS)


def test_driver_writes_the_sampled_change_table(tmp_path):
    from cafexp_amd import capi
    exe = os.path.join(ROOT, "cafexp_amd", "host", "cafexp_hip")
    assert os.path.exists(exe), "cafexp_hip missing: run __graft_entry__.build()"
    base = [exe, "-t", os.path.join(DATA, "mammals_tree.txt"), "-i", os.path.join(DATA, "mammal_gene_families.txt"), "-l", "0.0018", "--limit", "64"]
    out = _run(base + ["--sample-histories", "50", "--sample-seed", "7", "-o", str(tmp_path)])
    assert out.returncode == 0, out.stderr
    js = json.loads(out.stdout.strip().splitlines()[-1])
    assert js["histories"]["draws"] == 50 and js["histories"]["failed"] == 0 and js["histories"]["seconds"] >= 0
    pb, pr, _ = _mammals(**{"lambda": 0.0018})
    with _limit():
        ctx = capi.Context(pb)
        got = ctx.sample_histories(pr, 50, 7, sizes=False)
        ctx.close()
    with open(os.path.join(str(tmp_path), "Base_sampled_change.tab")) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip() and not ln.startswith("#")]
    ch, order, q = MR.children_of(pb), [], [MR.root_of(pb)]
    while q:
        v = q.pop(0)
        order.append(v)
        q.extend(ch[v])
    order = order[::-1]                                      # the reports' reverse level order
    assert len(rows) == pb.n_nodes
    for row, v in zip(rows, order):
        for cell, key in zip(row[1:4], ("n_increase", "n_decrease", "net_change")):
            mean, iv = cell.split(":")
            assert mean == "%.6g" % got[key][:, v].mean(), (v, key)
            lo, hi = (int(t) for t in re.fullmatch(r"(-?\d+)-(-?\d+)", iv).groups())
            srt = np.sort(got[key][:, v])                    # the marginal reports' rule on the draws' empirical CDF, level 0.95
            cdf = np.arange(1, 51) / 50.0
            assert (lo, hi) == (srt[np.argmax(cdf >= 0.025)], srt[np.argmax(cdf >= 0.975)]), (v, key)
    plain = _run(base)
    assert plain.returncode == 0 and "histories" not in json.loads(plain.stdout.strip().splitlines()[-1])
    for extra in (["--gpus", "2"], ["-b"]):
        bad = _run(base + extra + ["--sample-histories", "5"])
        assert bad.returncode != 0 and "--sample-histories" in bad.stderr
