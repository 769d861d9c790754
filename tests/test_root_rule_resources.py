"""The kernels of the sum rule -- K4's sum-rule kernel (leaf_reduce.hip), the per-family root kernel's (family_lambda.hip) --
and the two of cafe_root_posterior (root_posterior.hip) keep their sums, maxima and tile partials in registers and LDS.
Cross-compile each file for gfx950 (CPU only) and read the compiler's resource remarks: no kernel may use scratch or spill
vector registers (the rule `make check` applies)."""
import pytest

from helpers import kernel_resources

KERNELS = {
    "leaf_reduce.hip": ["root_reduce_sum_kernel"],
    "family_lambda.hip": ["family_root_sum_kernel"],
    "root_posterior.hip": ["root_posterior_column_kernel", "root_posterior_row_kernel"],
}


@pytest.mark.parametrize("hip_file", sorted(KERNELS))
def test_every_kernel_runs_without_scratch(hip_file):
    kernels = kernel_resources(hip_file)
    for k in KERNELS[hip_file]:
        mine = {n: v for n, v in kernels.items() if k in n}
        assert len(mine) == 1, (k, sorted(kernels))
        for n, res in mine.items():
            assert res["ScratchSize"] == 0, (n, res)
            assert res["VGPRs Spill"] == 0, (n, res)
    if hip_file == "root_posterior.hip":                     # nothing else in the file launches
        assert len([n for n in kernels if "root_posterior_" in n]) == len(KERNELS[hip_file]), sorted(kernels)
