"""The kernels of branch_scores.hip -- the Gram tile kernel (one 16 x 16 accumulator tile per wave, two 16 x 64 operand tiles in
LDS), the weighted row sum, the slab reduction and the panel's finish kernel -- keep what they carry in registers (or LDS).
Cross-compile the file for gfx950 (CPU only) and read the compiler's resource remarks: no kernel may use scratch or spill
vector registers (the rule `make check` applies).  The walk's kernels are gradient.hip's, pinned by
tests/test_gradient_resources.py; the GEMM is sum_product.hip's, pinned by tests/test_sum_product_resources.py."""
from helpers import kernel_resources

KERNELS = ["weighted_gram_tile_kernel", "weighted_gram_rowsum_kernel", "weighted_gram_reduce_kernel", "score_panel_finish_kernel"]


def test_every_kernel_runs_without_scratch():
    kernels = kernel_resources("branch_scores.hip")
    mine = {k: v for k, v in kernels.items() if "weighted_gram_" in k or "score_panel_" in k}
    for k in KERNELS:
        assert any(k in n for n in mine), k
    assert len(mine) == len(KERNELS), sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
