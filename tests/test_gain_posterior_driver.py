"""cafexp_hip --gain NU --gain-posterior on the first 80 families of tests/test_gain_driver.py's drawn table, rates fixed
(-l, --gain: nothing is searched).  Gain_origins.tab is held against the binding's cafe_gain_posterior call on the same table
at the same rates, to the 6 digits the cells are printed with (5e-6 relative); Gain_branch_origins.tab against the binding's
arrays summed in numpy over the table's families (1e-9 relative: the driver sums the distinct families times their
multiplicities, 12 digits are printed) and against the per-family lines of the first file (each cell is rounded to 6 digits:
5e-6 of the sum of the magnitudes)."""
import json
import os
import subprocess

import numpy as np
import pytest

import bd_lm_ref as R
import marginal_ref as MR
from cafexp_amd import problem as P
from test_events_driver import _read_tab, _reverse_level_order
from test_gain_driver import ABSENT, DRIVER, LAM, M, NU, RR, _problem, draw_table

FAMILIES = 80


def _cells(row, first, count):
    return np.array([[float(x) for x in cell.split(":")] for cell in row[first:first + count]])


@pytest.mark.gpu
def test_both_files_are_the_bindings_arrays_at_the_same_rates(tmp_path):
    from cafexp_amd import capi
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    counts = draw_table()[:FAMILIES]
    assert len(np.unique(counts, axis=0)) < len(counts)      # multiplicities above 1: the sums weigh the distinct entries
    tree, fams, out = tmp_path / "tree.txt", tmp_path / "families.txt", tmp_path / "out"
    tree.write_text(R.NEWICK + "\n")
    fams.write_text("Desc\tFamily ID\t" + "\t".join(R.SPECIES) + "\n" + "".join("(null)\tf%d\t%s\n" % (i, "\t".join(map(str, c))) for i, c in enumerate(counts)))
    r = subprocess.run([DRIVER, "-t", str(tree), "-i", str(fams), "-z", "-l", str(LAM), "--gain", str(NU), "--gain-posterior", "--root-absent", str(ABSENT),
                        "--sizes", "%d,%d" % (M, RR), "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["lambda"] == [LAM] and js["nu"] == NU and js["families"] == FAMILIES and js["gain_posterior_seconds"] >= 0

    pb = _problem(counts)
    pr = P.Params(lambdas=np.ones(1), prior=P.prior_uniform(RR))
    ctx = capi.Context(pb)
    try:
        got = ctx.gain_posterior(pr, np.arange(FAMILIES), np.full(FAMILIES, LAM), np.full(FAMILIES, LAM), np.full(FAMILIES, NU), ABSENT)
    finally:
        ctx.close()
    assert np.isfinite(got["lnl"]).all()

    order, root = _reverse_level_order(pb), MR.root_of(pb)
    branches = [v for v in order if v != root]
    n = pb.n_nodes
    head, rows = _read_tab(str(out / "Gain_origins.tab"))
    assert head[0] == "FamilyID" and len(head) == 2 * n and [r[0] for r in rows] == ["f%d" % i for i in range(FAMILIES)]
    assert head[1 + n:] == [head[1 + order.index(v)] + "^" for v in branches]
    printed = {k: np.full((FAMILIES, n), np.nan) for k in ("p_absent", "mean", "p_gain", "p_loss")}
    for f in range(FAMILIES):
        nodes, edges = _cells(rows[f], 1, n), _cells(rows[f], 1 + n, n - 1)
        printed["p_absent"][f, order], printed["mean"][f, order] = nodes[:, 0], nodes[:, 1]
        printed["p_gain"][f, branches], printed["p_loss"][f, branches] = edges[:, 0], edges[:, 1]
    for key, values in printed.items():
        assert np.array_equal(np.isnan(values), np.isnan(got[key])), key
        keep = ~np.isnan(values)
        worst = np.max(np.abs(values[keep] - got[key][keep]) - 5e-6 * np.abs(got[key][keep]))
        print("%s: largest excess over the printed digits %.3e" % (key, worst))
        assert worst <= 1e-300, key

    thead, trows = _read_tab(str(out / "Gain_branch_origins.tab"))
    assert thead[:5] == ["#Node", "originated", "lost", "present", "p_gain>0.5"] and "%d families; 0 failed" % FAMILIES in thead[5]
    assert [r[0] for r in trows[:-1]] == [head[1 + order.index(v)] for v in branches]
    for row, v in zip(trows[:-1], branches):
        for value, want, lines in ((float(row[1]), got["p_gain"][:, v], printed["p_gain"][:, v]), (float(row[2]), got["p_loss"][:, v], printed["p_loss"][:, v]),
                                   (float(row[3]), 1 - got["p_absent"][:, v], 1 - printed["p_absent"][:, v])):
            assert abs(value - want.sum()) <= 1e-9 * np.abs(want).sum() + 1e-300, (v, row)
            assert abs(value - lines.sum()) <= 5e-6 * (np.abs(lines).sum() + FAMILIES), (v, row)
        assert float(row[4]) == (got["p_gain"][:, v] > 0.5).sum()
    last = trows[-1]
    assert last[0] == "#Root " + head[1 + order.index(root)] and last[1] == "absent" and last[3] == "present"
    assert abs(float(last[2]) - got["p_absent"][:, root].sum()) <= 1e-9 * FAMILIES
    assert abs(float(last[2]) + float(last[4]) - FAMILIES) <= 1e-9 * FAMILIES
    assert abs(js["absent_at_root"] - float(last[2])) <= 1e-9 * FAMILIES
    assert js["families_with_a_likely_origin"] == (np.nanmax(got["p_gain"], axis=1) > 0.5).sum() >= 1


def test_refused_without_a_gain_option(tmp_path):
    assert os.path.exists(DRIVER), "cafexp_hip missing: run __graft_entry__.build()"
    r = subprocess.run([DRIVER, "-t", str(tmp_path / "no_tree.txt"), "-i", str(tmp_path / "no_families.txt"), "-o", str(tmp_path / "out"), "--gain-posterior"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--gain-posterior reports where families originated under the gain model: give --gain NU or --estimate-gain with it" in r.stderr
    assert not os.path.exists(str(tmp_path / "out"))
