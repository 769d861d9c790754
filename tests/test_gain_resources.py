"""The gain kernel (family_gain.hip: family_gain_kernel.h on SlotParamGain) keeps what the per-family kernel keeps in registers
-- a row of the recurrence, the powers of beta, the child's likelihood vector -- and evaluates row 0 once before the rows run.
The rule tests/test_family_lambda_lm_resources.py pins, on the new file: cross-compile for gfx950 (CPU only) and read the
compiler's resource remarks -- all twelve widths E = 2 .. 32 and both root kernels are there, and none uses scratch memory or
spills a vector register.  The file holds no instantiation of the kernels of the two older entries."""
import os

from helpers import CSRC, kernel_resources

WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]


def test_every_gain_instantiation_runs_without_scratch():
    kernels = kernel_resources("family_gain.hip")
    assert not [k for k in kernels if "family_lambda_kernel" in k or "family_root_kernel" in k or "family_root_sum_kernel" in k], sorted(kernels)
    mine = {k: v for k, v in kernels.items() if "family_gain_kernel" in k}
    for E in WIDTHS:
        assert any("family_gain_kernelILi%dEEE" % E in k for k in mine), E
    assert len(mine) == len(WIDTHS), sorted(mine)
    roots = {k: v for k, v in kernels.items() if "family_gain_root_" in k}
    assert len(roots) == 2 and any("root_sum_kernel" in k for k in roots), sorted(roots)
    for k, res in sorted({**mine, **roots}.items()):
        print(k, res.get("VGPRs"), res.get("AGPRs"), res.get("Occupancy"))
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)


def test_makefile_builds_and_checks_the_gain_kernel():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = next(ln for ln in mk.splitlines() if ln.startswith("SRC"))
    assert "family_gain.hip" in src.split() and "family_lambda.hip" in src.split() and "family_lambda_lm.hip" in src.split()
    check = mk[mk.index("\ncheck:"):]
    assert "family_gain.hip" in check.splitlines()[1].split()
    assert "-c family_gain.hip" in check
