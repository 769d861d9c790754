"""The engine of the posterior calls (sum_product.hip) -- the fp64 MFMA GEMM with its 8 accumulator tiles and register
prefetch, and the product kernel -- keeps everything in registers.  Cross-compile the file for gfx950 (CPU only) and read the
compiler's resource remarks: exactly the four GEMM instantiations and the product kernel are there, and none uses scratch or
spills a vector register (the rule `make check` applies)."""
from helpers import kernel_resources


def test_every_kernel_runs_without_scratch():
    kernels = kernel_resources("sum_product.hip")
    mine = {k: v for k, v in kernels.items() if "marginal_" in k}
    gemm = [k for k in mine if "marginal_gemm_kernel" in k]
    assert len(gemm) == 4, sorted(gemm)                      # up (store, multiply), down, split
    assert any("marginal_product_kernel" in n for n in mine)
    assert len(mine) == len(gemm) + 1 and len(kernels) == len(mine), sorted(kernels)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
