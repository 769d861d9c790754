"""cafexp_hip --expected-events on synth20: after the search the driver writes <Model>_expected_events.tab (gains:losses per
family and node, "-" at the root) and <Model>_branch_events.tab (per branch: gains, losses, net, turnover summed over the
table).  Both are recomputed from the binding's own cafe_expected_events arrays at the printed optimum: the cells to the
6 digits they are printed with (5e-6 relative), the per-branch totals, summed in numpy in family order, to 1e-8 relative as
tests/test_standard_errors_driver.py holds its numbers; net = gains - losses and turnover = gains + losses to the 12 digits of
the file."""
import json
import os
import subprocess

import numpy as np
import pytest

import marginal_ref as MR
from cafexp_amd import problem as P
from helpers import DATA, read, table

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "cafexp_amd", "host", "cafexp_hip")
COMMON = ["-t", os.path.join(DATA, "synth20_tree.txt"), "-i", os.path.join(DATA, "synth20_families.txt"), "-s", "7", "--expected-events"]


def _read_tab(path):
    with open(path) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    return rows[0], rows[1:]


def _reverse_level_order(pb):
    ch, order, q = MR.children_of(pb), [], [MR.root_of(pb)]
    while q:
        v = q.pop(0)
        order.append(v)
        q.extend(ch[v])
    return order[::-1]


@pytest.mark.gpu
@pytest.mark.parametrize("extra,model", [([], "Base"), (["-k", "2"], "Gamma"), (["--estimate-mu"], "Base")])
def test_the_tables_are_the_bindings_arrays_at_the_printed_optimum(tmp_path, extra, model):
    from cafexp_amd import capi
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([DRIVER] + COMMON + ["-o", str(tmp_path)] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["expected_events"]["failed"] == 0 and js["expected_events"]["seconds"] >= 0

    species, ids, counts = table("synth20_families.txt")
    pb = P.build_problem(P.parse_newick(read("synth20_tree.txt")), species, ids, counts)
    assert pb.n_families == js["n_families"] and pb.max_family_size == js["max_family_size"]
    pr = P.Params(lambdas=np.array(js["lambda"]), prior=P.prior_uniform(pb.max_root_family_size))
    K = 1
    if model == "Gamma":
        K = 2
        pr.multipliers, pr.cat_probs = np.array(js["multipliers"]), np.full(2, 0.5)
    ctx = capi.Context(pb, max_categories=K)
    try:
        if "mu" in js:
            ctx.set_death_rates(js["mu"])
        got = ctx.expected_events(pr, alpha=js.get("alpha", 1.0))
    finally:
        ctx.close()
    assert not got["failed"].any()

    order, root = _reverse_level_order(pb), MR.root_of(pb)
    head, rows = _read_tab(os.path.join(str(tmp_path), model + "_expected_events.tab"))
    assert head[0] == "FamilyID" and len(head) == 1 + pb.n_nodes and [r[0] for r in rows] == list(pb.family_ids)
    for f in range(pb.n_families):
        for col, v in enumerate(order):
            cell = rows[f][1 + col]
            if v == root:
                assert cell == "-"
                continue
            g, l = (float(x) for x in cell.split(":"))
            assert abs(g - got["gains"][f, v]) <= 5e-6 * got["gains"][f, v] + 1e-300, (f, v)
            assert abs(l - got["losses"][f, v]) <= 5e-6 * got["losses"][f, v] + 1e-300, (f, v)

    thead, trows = _read_tab(os.path.join(str(tmp_path), model + "_branch_events.tab"))
    assert thead[:5] == ["#Node", "gains", "losses", "net", "turnover"] and "%d families" % pb.n_families in thead[5]
    branches = [v for v in order if v != root]
    assert [r[0] for r in trows] == [head[1 + order.index(v)] for v in branches]
    for row, v in zip(trows, branches):
        g, l, net, turn = (float(x) for x in row[1:5])
        wg, wl = got["gains"][:, v].sum(), got["losses"][:, v].sum()
        assert abs(g - wg) <= 1e-8 * wg and abs(l - wl) <= 1e-8 * wl, (v, g, wg, l, wl)
        assert abs(net - (g - l)) <= 1e-11 * (g + l) and abs(turn - (g + l)) <= 1e-11 * (g + l)
        assert g > 0 and l > 0


def test_the_driver_refuses_what_does_not_combine(tmp_path):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    common = COMMON + ["-o", str(tmp_path / "out")]
    for extra, message in ((["-b"], "-b is not supported with it"), (["--gpus", "2"], "--gpus is not supported with it"),
                           (["--simulate", "10", "-l", "0.01"], "--simulate is not supported with it")):
        r = subprocess.run([DRIVER] + common + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--expected-events" in r.stderr and message in r.stderr, (extra, r.stderr)
    assert not os.path.exists(str(tmp_path / "out"))
