"""The two-rate K1 (bd_matrix_lm.hip: the body of bd_matrix_build.h on SlotParamLM, separate birth and death rates) keeps every
row of its recurrence in registers exactly as the lambda = mu instantiation does, with one more constant live.  The rule
tests/test_k1_resources.py pins for bd_matrix.hip, on this file: cross-compile for gfx950 (CPU only), read the compiler's
resource remarks -- every width 2 .. 32 in both layouts and in the two-pool launch is there, and none uses scratch memory or
spills a vector register.  No kernel of the file is a lambda = mu instantiation (that test counts them by the slot type)."""
import os

from helpers import CSRC, kernel_resources

WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]


def test_every_two_rate_k1_instantiation_runs_without_scratch():
    kernels = kernel_resources("bd_matrix_lm.hip")
    assert not [k for k in kernels if "bd_matrix_build" in k and "SlotParamLM" not in k], sorted(kernels)
    k1 = {k: v for k, v in kernels.items() if "bd_matrix_build" in k}
    for E in WIDTHS:
        assert "_ZN4cafe27bd_matrix_build_both_kernelINS_11SlotParamLMELi%dEEEv" % E in "|".join(k1), E
        for km in (0, 1):
            assert "_ZN4cafe22bd_matrix_build_kernelINS_11SlotParamLMELi%dELb%dEEEv" % (E, km) in "|".join(k1), (E, km)
    assert len(k1) == 3 * len(WIDTHS), sorted(k1)
    for k, res in k1.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)


def test_makefile_builds_and_checks_the_two_rate_kernel():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = next(ln for ln in mk.splitlines() if ln.startswith("SRC"))
    assert "bd_matrix_lm.hip" in src.split()
    check = mk[mk.index("\ncheck:"):]
    assert "-c bd_matrix_lm.hip" in check
