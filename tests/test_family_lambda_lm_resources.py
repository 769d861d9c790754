"""The two-rate per-family kernel (family_lambda_lm.hip: the body of family_lambda_kernel.h on SlotParamLM) keeps a row of the
recurrence, the powers of beta and the child's likelihood vector in registers exactly as family_lambda.hip does, with one more
constant live.  The rule tests/test_family_lambda_resources.py pins for that file, on the new one: cross-compile for gfx950 (CPU
only) and read the compiler's resource remarks -- all twelve widths E = 2 .. 32 are there, and none uses scratch memory or
spills a vector register.  The file holds no lambda = mu instantiation and no root kernel (that test counts them)."""
import os

from helpers import CSRC, kernel_resources

WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]


def test_every_two_rate_instantiation_runs_without_scratch():
    kernels = kernel_resources("family_lambda_lm.hip")
    assert not [k for k in kernels if ("family_lambda_kernel" in k and "SlotParamLM" not in k) or "family_root_kernel" in k], sorted(kernels)
    mine = {k: v for k, v in kernels.items() if "family_lambda_kernel" in k}
    for E in WIDTHS:
        assert any("family_lambda_kernelINS_11SlotParamLMELi%dEEE" % E in k for k in mine), E
    assert len(mine) == len(WIDTHS), sorted(mine)
    for k, res in sorted(mine.items()):
        print(k, res.get("VGPRs"), res.get("Occupancy"))
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)


def test_makefile_builds_and_checks_the_two_rate_kernel():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = next(ln for ln in mk.splitlines() if ln.startswith("SRC"))
    assert "family_lambda_lm.hip" in src.split() and "family_lambda.hip" in src.split()
    check = mk[mk.index("\ncheck:"):]
    assert "family_lambda_lm.hip" in check.splitlines()[1].split()
    assert "-c family_lambda_lm.hip" in check
