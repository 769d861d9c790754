"""The kernels of branch_change.hip -- the band kernel with its block of 8 accumulators, its register window of B rows and its
LDS tile, the tail GEMM with its 8 accumulator tiles and register prefetch, the leaf walk, the sums and the finish -- keep
everything in registers.  Cross-compile the file for gfx950 (CPU only) and read the compiler's resource remarks: exactly the seven
change_ kernels are there, and none uses scratch or spills a vector register -- the rule `make check` applies, whose line for this
file is pinned here.  sum_product.hip keeps its GEMM instantiations: the tail GEMM is a kernel of this file."""
import os
import re

from helpers import CSRC, kernel_resources

KERNELS = ["change_root_kernel", "change_band_kernel", "change_tail_gemm_kernel", "change_colsum_kernel", "change_leaf_kernel",
           "change_node_mean_kernel", "change_finish_kernel"]


def test_every_kernel_runs_without_scratch():
    kernels = kernel_resources("branch_change.hip")
    mine = {k: v for k, v in kernels.items() if "change_" in k}
    for k in KERNELS:
        assert any(k in n for n in mine), k
    assert len(mine) == len(KERNELS) and len(kernels) == len(mine), sorted(kernels)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
    band = next(v for k, v in mine.items() if "change_band_kernel" in k)
    assert band["VGPRs"] <= 128, band                         # at least four waves per SIMD: the launches hide their own latency


def test_the_makefile_builds_and_checks_the_file():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\bbranch_change\.hip\b", text, re.M)
    assert re.search(r"^check:.*\bbranch_change\.hip\b", text, re.M)
    assert "$(call resource_check,-c branch_change.hip,change_,0,0)" in text


def test_the_engine_is_untouched():
    text = open(os.path.join(CSRC, "sum_product.hip")).read()
    assert "change_" not in text and "branch_change" not in text
    assert len(re.findall(r"^template int launch_gemm<", text, re.M)) == 3
