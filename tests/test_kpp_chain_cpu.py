"""csrc/kpp_chain.h and csrc/kpp_layout.h on the host: k-means++'s walk restated
serially from the header's functions against the plain chain s = s + q, every
prefix sum bit for bit (random rows, ties that round both ways, wrong guesses,
inf / NaN rows, zeros and tiny sums, two crossings in one chunk, a row above the
binade, lengths 1 / 512 / 513 / 1537), and the workspace map against the byte
count lshkm_kpp_shard_ws_bytes has always returned (regions in order, disjoint,
aligned)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kpp_chain(tmp_path):
    exe = tmp_path / "kpp_chain_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "kpp_chain_check.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
