"""CPU: csrc/tile.h's derived bounds FU_A1H (hash tile) and FU_A1 (3-product
tile) against a host model of the tiles' arithmetic, tests/window_model_check.cpp
(a stand-alone program; nothing is loaded into Python): the split of x and v
into f16 parts, exact f32 products, each MFMA's 17 operands summed in several
orders with every addition rounded toward zero, up, down or to nearest, the
hash tile's 8 steps added in f32. It asserts the bound on random full-mantissa
vectors, one-signed vectors, f16 ties with subnormal lo parts and rows at the
f16 range guard, and the converse on adversarial vectors: half the constant is
exceeded, so the model can tell a bound that is too small."""
import os
import re
import subprocess

import window_bounds as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def build(tmp_path, extra=()):
    exe = str(tmp_path / "window_model_check")
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", *extra,
           os.path.join(ROOT, "tests", "window_model_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_tile_bounds_hold_and_bite(tmp_path):
    out = subprocess.run([build(tmp_path), "2000"], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
    # the tests' restatement (window_bounds.py) is the header's value, bit for bit
    m = re.search(r"FU_A1H=(\S+) .* FU_A1=(\S+) .* FU_A2=(\S+)", out.stdout)
    assert m, out.stdout
    assert [float.fromhex(g) for g in m.groups()] == [wb.FU_A1H, wb.FU_A1, wb.FU_A2]
    assert wb.FU_A1H < wb.FU_A1H_PARENT and wb.FU_A1 < wb.FU_A1_PARENT


def test_model_under_asan_ubsan(tmp_path):
    exe = build(tmp_path, ("-g", "-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "bad=0" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
