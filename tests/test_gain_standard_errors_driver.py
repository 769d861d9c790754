"""cafexp_hip --estimate-gain --gain-dense --standard-errors on the drawn table of tests/test_gain_driver.py: Gain_standard_errors.txt is,
to 1e-8 relative, the inverse outer-product matrix computed in numpy from the binding's cafe_gain_score_gradient scores at the printed
optimum, a family's score being s_f + (p / (1 - p)) s_absent with p = exp(lnl_absent) (tests/test_standard_errors_driver.py's check).
Without --gain-dense the option stays refused."""
import json
import subprocess
from contextlib import closing

import numpy as np
import pytest

import bd_lm_ref as R
from cafexp_amd import problem as P
from test_gain_driver import ABSENT, DRIVER, M, RR, _problem, draw_table
from test_standard_errors_driver import _parse


@pytest.mark.gpu
def test_standard_errors_are_the_inverse_outer_product_of_the_conditional_scores(tmp_path):
    from cafexp_amd import capi
    counts = draw_table()
    tree, fams, out = tmp_path / "tree.txt", tmp_path / "families.txt", tmp_path / "out"
    tree.write_text(R.NEWICK + "\n")
    fams.write_text("Desc\tFamily ID\t" + "\t".join(R.SPECIES) + "\n" + "".join("(null)\tf%d\t%s\n" % (i, "\t".join(map(str, c))) for i, c in enumerate(counts)))
    common = [DRIVER, "-t", str(tree), "-i", str(fams), "-z", "--estimate-gain", "--standard-errors", "--root-absent", str(ABSENT), "--sizes",
              "%d,%d" % (M, RR), "-s", "3", "-o", str(out)]
    refused = subprocess.run(common, capture_output=True, text=True, timeout=300)
    assert refused.returncode == 1 and "the posterior reports are not ported to the gain model: --standard-errors, --expected-events" in refused.stderr
    r = subprocess.run(common + ["--gain-dense"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    names, tab, corr, total = _parse(str(out / "Gain_standard_errors.txt"))
    assert names == ["Lambda", "Nu"] == js["standard_errors"]["parameters"] and np.all(tab[:, 1] > 0)
    pb = _problem(counts)
    with closing(capi.Context(pb)) as ctx:
        g = ctx.gain_score_gradient(P.Params(lambdas=np.ones(1), prior=P.prior_uniform(RR)), list(range(len(counts))) + [-1], js["lambda"], None, [js["nu"]], ABSENT)
    p = np.exp(g["lnl"][-1])
    S = np.stack([g["d_lambda"][:, 0], g["d_nu"][:, 0]], axis=1)
    S = S[:-1] + p / (1 - p) * S[-1]
    want = np.sqrt(np.diag(np.linalg.inv(S.T @ S)))
    print("SE", tab[:, 1], "numpy", want, "total score", total)
    assert np.all(np.abs(tab[:, 1] - want) <= 1e-8 * want)
    assert np.allclose(total, S.sum(axis=0), rtol=1e-8, atol=1e-8 * np.sqrt(np.trace(S.T @ S)))
