"""csrc/lshpc_layout.h on the host, lshkm_cube_p_closest's part: the cube
route's edges (d 128 / 129, k 30 / 31, P 447 / 448, forced lists) and the
screen's candidacy test (popcount shells and a bit-reversed compare at the
boundary shell) against probe_masks enumerated literally, for every k in 1..16,
every vertex difference y < 2^k and probes in {-1, 0, 1, 2, 3, k - 1, k, k + 1,
k + 2, C(k, 2) + k - 1, C(k, 2) + k, C(k, 2) + k + 1, 2^k - 2, 2^k - 1, 2^k,
2^k + 1, INT_MAX}; every probes of the k = 5 and k = 7 cubes; one partial shell
of the k = 30 cube."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cubepc_layout(tmp_path):
    exe = tmp_path / "cubepc_layout_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cubepc_layout_check.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
