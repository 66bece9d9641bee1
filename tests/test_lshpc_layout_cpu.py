"""csrc/lshpc_layout.h on the host: lshkm_lsh_p_closest's routing rule with its
edges (d 128 / 129, L * k 32 / 33, P 447 / 448), the kept-list capacities, every
plan's row segments (covering, none empty) and user chunks, and the chunk
workspace's regions (in order, disjoint, aligned, within the budget), for the
product's budget and the test build's 1 MiB (LSHKM_LSHPC_BUDGET=small)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lshpc_layout(tmp_path):
    exe = tmp_path / "lshpc_layout_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "lshpc_layout_check.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
