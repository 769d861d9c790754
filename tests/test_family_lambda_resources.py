"""The per-family kernel (family_lambda.hip: the body of family_lambda_kernel.h on SlotParam) keeps a row of the recurrence, the powers of a and the child's likelihood vector
in registers: a lane owns E columns, E = 2 .. 32 by matrix order.  Cross-compile it for gfx950 (CPU only) and read the
compiler's resource remarks: no instantiation may use scratch or spill vector registers (the rule test_k1_resources.py
pins for K1, whose row step it shares through bd_row.h)."""
from helpers import kernel_resources

WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]


def test_every_instantiation_runs_without_scratch():
    kernels = kernel_resources("family_lambda.hip")
    mine = {k: v for k, v in kernels.items() if "family_lambda_kernel" in k or "family_root_kernel" in k}
    for E in WIDTHS:
        assert any("family_lambda_kernelINS_9SlotParamELi%dEEE" % E in k for k in mine), E
    assert len(mine) == len(WIDTHS) + 1, sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
