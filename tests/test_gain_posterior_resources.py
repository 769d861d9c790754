"""The down kernel of cafe_gain_posterior (family_gain_posterior.hip: family_gain_down_kernel.h) keeps a row of the recurrence,
its accumulator, the step's partial sums and the powers of beta in registers, as the up kernel keeps the row and the child's
likelihood vector.  The rule tests/test_gain_resources.py pins, on the new file: cross-compile for gfx950 (CPU only) and read the
compiler's resource remarks -- all twelve widths E = 2 .. 32 are there, and none uses scratch memory or spills a vector
register.  The file holds no instantiation of the up pass's kernels: it calls family_gain.hip's."""
import os

from helpers import CSRC, kernel_resources

WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]


def test_every_down_instantiation_runs_without_scratch():
    kernels = kernel_resources("family_gain_posterior.hip")
    assert not [k for k in kernels if "family_gain_kernel" in k or "family_gain_root_" in k or "family_lambda_kernel" in k], sorted(kernels)
    mine = {k: v for k, v in kernels.items() if "family_gain_down_kernel" in k}
    for E in WIDTHS:
        assert any("family_gain_down_kernelILi%dEEE" % E in k for k in mine), E
    assert len(mine) == len(WIDTHS), sorted(mine)
    roots = {k: v for k, v in kernels.items() if "family_gain_down_root_kernel" in k}
    assert len(roots) == 1, sorted(roots)
    for k, res in sorted({**mine, **roots}.items()):
        print(k, res.get("VGPRs"), res.get("AGPRs"), res.get("Occupancy"))
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)


def test_makefile_builds_and_checks_the_down_kernel():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = next(ln for ln in mk.splitlines() if ln.startswith("SRC"))
    assert "family_gain_posterior.hip" in src.split() and "family_gain.hip" in src.split()
    rule = next(ln for ln in mk.splitlines() if ln.startswith("%.o:"))
    assert "family_gain_down_kernel.h" in rule.split()
    check = mk[mk.index("\ncheck:"):]
    assert "family_gain_posterior.hip" in check.splitlines()[1].split() and "family_gain_down_kernel.h" in check.splitlines()[1].split()
    assert "-c family_gain_posterior.hip,family_gain_down_,0,0" in check
