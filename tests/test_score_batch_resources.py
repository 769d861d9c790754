"""The two kernels of root_reduce_batch.hip -- K4 and the final sum of a batch of parameter vectors -- keep everything in
registers and LDS.  Cross-compile the file for gfx950 (CPU only) and read the compiler's resource remarks: exactly the two
kernels are there, and neither uses scratch or spills a vector register -- the rule `make check` applies, whose line for this
file is pinned here.  The per-family arithmetic is root_family.h's: the single-call kernels of leaf_reduce.hip keep their names
and call the same functions."""
import os
import re

from helpers import CSRC, kernel_resources

KERNELS = ["root_reduce_batch_kernel", "final_sum_batch_kernel"]


def test_every_kernel_runs_without_scratch():
    kernels = kernel_resources("root_reduce_batch.hip")
    for k in KERNELS:
        assert any(k in n for n in kernels), k
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for k, res in kernels.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)


def test_the_makefile_builds_and_checks_the_file():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\broot_reduce_batch\.hip\b", text, re.M)
    assert re.search(r"^check:.*\broot_reduce_batch\.hip\b", text, re.M)
    assert "$(call resource_check,-c root_reduce_batch.hip,(root_reduce|final_sum)_batch_,0,0)" in text
    assert re.search(r"^%\.o:.*\broot_family\.h\b", text, re.M)


def test_the_single_call_kernels_share_the_arithmetic():
    single = open(os.path.join(CSRC, "leaf_reduce.hip")).read()
    batch = open(os.path.join(CSRC, "root_reduce_batch.hip")).read()
    for name in ("root_reduce_kernel", "root_reduce_sum_kernel", "partial_sum_kernel"):
        assert re.search(r"__global__ __launch_bounds__\(256\) void %s\(" % name, single), name
    for fn in ("family_base_max", "family_gamma_max", "family_gamma_sum", "final_sum_block"):
        assert fn + "(" in single and fn + "(" in batch, fn
    assert "column_log_sum(" in single and "column_log_sum(" in batch
    leaf = kernel_resources("leaf_reduce.hip")
    for name in ("root_reduce_kernel", "root_reduce_sum_kernel", "partial_sum_kernel"):
        res = next(v for k, v in leaf.items() if name in k)
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (name, res)
