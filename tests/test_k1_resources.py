"""K1 (bd_matrix.hip: the body of bd_matrix_build.h on SlotParam) keeps every row of its recurrence in registers: a lane owns E columns, E = 2 .. 32 by matrix order.
At E = 24 the kernel uses all 256 VGPRs and at E = 28 / 32 it also needs AGPRs, so a small change to the row step could push
the widest variants to scratch memory without any value changing.  Cross-compile the kernel for gfx950 (CPU only) and read
the compiler's resource remarks: no K1 instantiation may use scratch or spill vector registers."""
from helpers import kernel_resources

WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]


def test_every_k1_instantiation_runs_without_scratch():
    kernels = kernel_resources("bd_matrix.hip")
    k1 = {k: v for k, v in kernels.items() if "bd_matrix_build" in k}
    # every width in both single-pool layouts (row-major, k-major) and in the scorer's two-pool launch
    for E in WIDTHS:
        assert "_ZN4cafe27bd_matrix_build_both_kernelINS_9SlotParamELi%dEEEv" % E in "|".join(k1), E
        for km in (0, 1):
            assert "_ZN4cafe22bd_matrix_build_kernelINS_9SlotParamELi%dELb%dEEEv" % (E, km) in "|".join(k1), (E, km)
    assert len(k1) == 3 * len(WIDTHS), sorted(k1)
    for k, res in k1.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
