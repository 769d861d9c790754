"""The kernels of history.hip -- the prefix walks with eight products in flight per lane, the LDS count reduction and the
transpose -- keep everything in registers.  Cross-compile the file for gfx950 (CPU only) and read the compiler's resource
remarks: no history_* kernel may use scratch or spill vector registers (the rule `make check` applies)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cafexp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ["history_rootz_kernel", "history_z_kernel", "history_category_kernel", "history_root_kernel", "history_node_kernel",
           "history_leaf_kernel", "history_count_kernel", "history_transpose_kernel"]


def _flags():
    with open(os.path.join(CSRC, "Makefile")) as f:
        line = next(ln for ln in f if ln.startswith("FLAGS"))
    return line.split(":=", 1)[1].replace("$(ARCH)", "gfx950").split()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_history_kernel_runs_without_scratch(tmp_path):
    r = subprocess.run([HIPCC] + _flags() + ["-Rpass-analysis=kernel-resource-usage", "-c", "history.hip", "-o", str(tmp_path / "h.o")],
                       cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
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
