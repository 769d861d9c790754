"""The kernels of gradient.hip -- the root, scan, weighted-dot, leaf-filter, leaf-sum and finish kernels of
cafe_score_gradient -- keep their recurrences in registers (the leaf filter its three tiles in LDS).  Cross-compile the file
for gfx950 (CPU only) and read the compiler's resource remarks: no kernel may use scratch or spill vector registers (the
rule `make check` applies).  The GEMM is sum_product.hip's, pinned by tests/test_sum_product_resources.py."""
from helpers import kernel_resources

KERNELS = ["gradient_root_kernel", "gradient_scan_kernel", "gradient_dot_kernel", "gradient_leaf_filter_kernel", "gradient_leaf_kernel",
           "gradient_finish_kernel"]


def test_every_kernel_runs_without_scratch():
    kernels = kernel_resources("gradient.hip")
    mine = {k: v for k, v in kernels.items() if "gradient_" in k}
    for k in KERNELS:
        assert any(k in n for n in mine), k
    assert len(mine) == len(KERNELS), sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
