"""The kernels that marginal.hip keeps for its own call -- root, column-sum, leaf and the two summary kernels -- keep everything
in registers.  Cross-compile the file for gfx950 (CPU only) and read the compiler's resource remarks: no kernel may use
scratch or spill vector registers (the rule `make check` applies).  The GEMM and the product kernel are sum_product.hip's,
pinned by tests/test_sum_product_resources.py."""
from helpers import kernel_resources

SMALL = ["marginal_root_kernel", "marginal_colsum_kernel", "marginal_leaf_kernel", "marginal_summary_kernel", "marginal_leaf_summary_kernel"]


def test_every_kernel_runs_without_scratch():
    kernels = kernel_resources("marginal.hip")
    mine = {k: v for k, v in kernels.items() if "marginal_" in k}
    assert not [k for k in mine if "marginal_gemm_kernel" in k or "marginal_product_kernel" in k], sorted(mine)
    for k in SMALL:
        assert any(k in n for n in mine), k
    assert len(mine) == len(SMALL), sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
