"""The kernels of predictive.hip -- the fp64 MFMA GEMM of a leaf branch with its 8 accumulator tiles and register prefetch, the
sums over the predictive distribution and their finish -- keep everything in registers.  Cross-compile the file for gfx950 (CPU
only) and read the compiler's resource remarks: exactly the three predictive_ kernels are there (the K-range variant of the GEMM
was not built), and none uses scratch or spills a vector register -- the rule `make check` applies, whose line for this file is
pinned here; tests/test_history_resources.py runs `make check` itself.  sum_product.hip keeps its four GEMM instantiations: the
new GEMM is not one of them."""
import os
import re

from helpers import CSRC, kernel_resources

KERNELS = ["predictive_gemm_kernel", "predictive_sums_kernel", "predictive_finish_kernel"]


def test_every_kernel_runs_without_scratch():
    kernels = kernel_resources("predictive.hip")
    mine = {k: v for k, v in kernels.items() if "predictive_" in k}
    for k in KERNELS:
        assert any(k in n for n in mine), k
    assert len(mine) == len(KERNELS) and len(kernels) == len(mine), sorted(kernels)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)


def test_the_makefile_builds_and_checks_the_file():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\bpredictive\.hip\b", text, re.M)
    assert re.search(r"^check:.*\bpredictive\.hip\b", text, re.M)
    assert "$(call resource_check,-c predictive.hip,predictive_,0,0)" in text


def test_the_engine_keeps_its_four_gemm_instantiations():
    text = open(os.path.join(CSRC, "sum_product.hip")).read()
    assert "predictive" not in text
    launches = re.findall(r"marginal_gemm_kernel<(\w+), (\w+)>", text)
    assert sorted(set(launches)) == [("MODE", "false"), ("kUp", "true")]      # up multiply; up store, down, split through MODE
    assert len(re.findall(r"^template int launch_gemm<", text, re.M)) == 3
