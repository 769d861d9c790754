"""The kernels of history.hip -- the prefix walks with eight products in flight per lane, the LDS count reduction and the
transpose -- keep everything in registers.  Cross-compile the file for gfx950 (CPU only) and read the compiler's resource
remarks: no history_* kernel may use scratch or spill vector registers (the rule `make check` applies)."""
import os
import subprocess

import pytest

from helpers import CSRC, HIPCC, kernel_resources

KERNELS = ["history_rootz_kernel", "history_z_kernel", "history_category_kernel", "history_root_kernel", "history_node_kernel",
           "history_leaf_kernel", "history_count_kernel", "history_transpose_kernel"]


def test_every_history_kernel_runs_without_scratch():
    kernels = kernel_resources("history.hip")
    mine = {k: v for k, v in kernels.items() if "history_" in k}
    for k in KERNELS:
        assert any(k in n for n in mine), k
    assert len(mine) == len(KERNELS), sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_make_check_passes():
    r = subprocess.run(["make", "-s", "-C", CSRC, "check", "HIPCC=" + HIPCC], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
