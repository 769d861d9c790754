"""The per-family kernel (family_lambda.hip: the body of family_lambda_kernel.h on SlotParam) keeps a row of the recurrence, the powers of a and the child's likelihood vector
in registers: a lane owns E columns, E = 2 .. 32 by matrix order.  Cross-compile it for gfx950 (CPU only) and read the
compiler's resource remarks: no instantiation may use scratch or spill vector registers (the rule test_k1_resources.py
pins for K1, whose row step it shares through bd_row.h)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cafexp_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32]


def _flags():
    with open(os.path.join(CSRC, "Makefile")) as f:
        line = next(ln for ln in f if ln.startswith("FLAGS"))
    return line.split(":=", 1)[1].replace("$(ARCH)", "gfx950").split()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_instantiation_runs_without_scratch(tmp_path):
    r = subprocess.run([HIPCC] + _flags() + ["-Rpass-analysis=kernel-resource-usage", "-c", "family_lambda.hip", "-o", str(tmp_path / "fl.o")],
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
    mine = {k: v for k, v in kernels.items() if "family_lambda_kernel" in k or "family_root_kernel" in k}
    for E in WIDTHS:
        assert any("family_lambda_kernelINS_9SlotParamELi%dEEE" % E in k for k in mine), E
    assert len(mine) == len(WIDTHS) + 1, sorted(mine)
    for k, res in mine.items():
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)
