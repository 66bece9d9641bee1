"""csrc/exact_layout.h on the host: the exact pass's routing rule against the
predicates it replaced (cosine x fp64 x switch x d 1..257 x K 1..1100) and at its
edges (K 256 / 257, 1024 / 1025, d 256 / 257), each form's workspace against the
extent its kernels touch (the fp64 CT's formula is 32 B short of the pruned
form's 2080 B at d = 1, K = 256), the regions (in order, disjoint, aligned) and
the grids."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_layout(tmp_path):
    exe = tmp_path / "exact_layout_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "exact_layout_check.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
