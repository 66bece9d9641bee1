"""Host check of the settled rows' candidate sets (no GPU needed):
csrc/settle.h's mask-bit to centroid map, the row's set from its two lanes'
masks and the k-th candidate, over all 256 positions."""
import os
import subprocess

import pytest

from amd import ROOT


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitized"])
def test_settle_masks(tmp_path, flags):
    # a stand-alone program, so the sanitizers run on it as they are
    exe = tmp_path / "settle_mask_check"
    subprocess.run(["g++", "-O1", "-std=c++17", *flags, "-o", str(exe),
                    os.path.join(ROOT, "tests", "settle_mask_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
