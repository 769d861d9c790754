"""The two-rate per-family kernel (family_lambda_lm.hip: the body of family_lambda_kernel.h on SlotParamLM) keeps a row of the
recurrence, the powers of beta and the child's likelihood vector in registers exactly as family_lambda.hip does, with one more
constant live.  The rule tests/test_family_lambda_resources.py pins for that file, on the new one: cross-compile for gfx950 (CPU
only) and read the compiler's resource remarks -- all twelve widths E = 2 .. 32 are there, and none uses scratch memory or
spills a vector register.  The file holds no lambda = mu instantiation and no root kernel (that test counts them)."""
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
def test_every_two_rate_instantiation_runs_without_scratch(tmp_path):
    r = subprocess.run([HIPCC] + _flags() + ["-Rpass-analysis=kernel-resource-usage", "-c", "family_lambda_lm.hip", "-o", str(tmp_path / "fllm.o")],
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
    assert not [k for k in kernels if ("family_lambda_kernel" in k and "SlotParamLM" not in k) or "family_root_kernel" in k], sorted(kernels)
    mine = {k: v for k, v in kernels.items() if "family_lambda_kernel" in k}
    for E in WIDTHS:
        assert any("family_lambda_kernelINS_11SlotParamLMELi%dEEE" % E in k for k in mine), E
    assert len(mine) == len(WIDTHS), sorted(mine)
    for k, res in sorted(mine.items()):
        print(k, res.get("VGPRs"), res.get("Occupancy"))
        assert res["ScratchSize"] == 0, (k, res)
        assert res["VGPRs Spill"] == 0, (k, res)


def test_makefile_builds_and_checks_the_two_rate_kernel():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = next(ln for ln in mk.splitlines() if ln.startswith("SRC"))
    assert "family_lambda_lm.hip" in src.split() and "family_lambda.hip" in src.split()
    check = mk[mk.index("\ncheck:"):]
    assert "family_lambda_lm.hip" in check.splitlines()[1].split()
    assert "-c family_lambda_lm.hip" in check
