"""K2 (prune_gemm.hip) lives on its register and LDS budget: the accumulators of a wave must stay in VGPRs (demoted to scratch
memory the kernel is five times slower), and the variants with 12-deep K tiles and row tiles of up to 80 rows are built for
FOUR workgroups per CU -- 128 VGPRs and, in 1 280-byte granules, a quarter of the CU's 160 KB of LDS each.  Cross-compile
the kernel for gfx950 (CPU only) and read the compiler's resource remarks, as `make check` does."""
import re

import pytest

from helpers import kernel_resources

MAX_SPILLED_VGPRS, MAX_SCRATCH_BYTES = 8, 64               # the limits of `make check`


@pytest.fixture(scope="module")
def k2_kernels():
    kernels = kernel_resources("prune_gemm.hip")
    # _ZN4cafe17prune_gemm_kernelILi<KB>ELi<MI>ELb<MUL>ELi<LEAF>ELb<TRANS>EEEvNS_8GemmArgsE
    k2 = {}
    for k, v in kernels.items():
        m = re.match(r"_ZN4cafe17prune_gemm_kernelILi(\d+)ELi(\d+)ELb([01])ELi(\d+)ELb([01])EEEv", k)
        if m:
            k2[tuple(int(x) for x in m.groups())] = v
    return k2


VARIANTS = [(0, 0, 0), (0, 1, 0), (0, 3, 0), (1, 0, 0), (1, 1, 0), (1, 3, 0), (0, 2, 0), (0, 0, 1)]   # (MUL, LEAF, TRANS)


def test_depth_12_tiles_of_up_to_80_rows_fit_four_workgroups_per_cu(k2_kernels):
    for mi in (2, 3, 4, 5):
        for var in VARIANTS:
            res = k2_kernels.get((12, mi) + var)
            assert res is not None, (mi, var)
            assert res["LDS Size"] <= 40960, (mi, var, res)
            assert res["VGPRs"] <= 128, (mi, var, res)
            assert res["Occupancy"] == 4, (mi, var, res)
            assert res["VGPRs Spill"] <= MAX_SPILLED_VGPRS, (mi, var, res)


def test_no_k2_instantiation_keeps_its_accumulators_in_scratch(k2_kernels):
    depths = sorted({k[0] for k in k2_kernels})
    assert depths == [8, 12, 16]
    assert len(k2_kernels) == len(depths) * 8 * len(VARIANTS), sorted(k2_kernels)
    for key, res in k2_kernels.items():
        assert res["ScratchSize"] <= MAX_SCRATCH_BYTES, (key, res)
        assert res["VGPRs Spill"] <= MAX_SPILLED_VGPRS, (key, res)
