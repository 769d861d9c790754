"""The passes in front of the prune (extents.hip: magnitude tables, the per-level interval / bound kernel, the K ranges, the
tile planner) are latency-bound kernels that live on many resident waves.  Cross-compile the file for gfx950 (CPU only) and
read the compiler's resource remarks: no kernel may use scratch memory or spill a vector register, and the level kernel's
static LDS stays inside the budget it was laid out for.

The budget: node_level_kernel is launched with 256 threads and runs FIVE workgroups per CU (20 waves, five per SIMD: its
loops wait on memory round trips, and the waves of the other workgroups fill them).  Five waves per SIMD allow a lane
512 / 5 = 102 vector registers, 96 in the granule the register file is dealt in -- the list loops hold a batch of 16 loads,
the k-step sum a batch of 4 and a running maximum and sum for each of the workgroup's four column tiles -- and a CU of
gfx950 has 160 KB (163 840 bytes) of LDS, so five workgroups leave each 32 768 bytes.  What the kernel declares, with
kLevelTiles = 4 column tiles per workgroup and kMaxSteps = 512 steps: s_acc 4 x 512 x 4 = 8 192, s_cb 512 x 16 = 8 192, the
distinct lists 4 x 128 x 4 = 2 048, their bitmaps 4 x 64 x 4 = 1 024, the partial sums of the four waves
2 x 4 x 4 x 64 x 4 = 8 192, the matrix extents of up to four interior children 4 x 256 x 4 = 4 096 -- 31 744 -- and 192 bytes
of scalars: 31 936.  A fifth array of that size, a fifth tile per workgroup or a register count past 96 would cost a resident
workgroup -- that is what the bounds below are there to catch."""
from helpers import kernel_resources

LDS_PER_CU = 160 * 1024
LEVEL_WORKGROUPS_PER_CU = 5


def test_no_prepass_kernel_uses_scratch_and_the_level_kernel_keeps_its_lds_budget():
    kernels = kernel_resources("extents.hip")
    names = "|".join(kernels)
    for want in ("mag_tables_kernel", "node_level_kernel", "range_kernel", "tile_plan_kernel"):
        assert want in names, (want, sorted(kernels))
    assert len(kernels) == 4, sorted(kernels)
    for k, res in kernels.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
    level = next(res for k, res in kernels.items() if "node_level_kernel" in k)
    print("node_level_kernel:", level)
    assert level["LDS Size"] <= LDS_PER_CU // LEVEL_WORKGROUPS_PER_CU == 32768, level
    assert level["VGPRs"] + level["AGPRs"] <= 96, level
    assert level["Occupancy"] >= LEVEL_WORKGROUPS_PER_CU, level
