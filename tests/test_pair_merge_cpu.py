"""Host checks of the fused refinement's pair naming (no GPU needed):
csrc/pair_merge.h against a sort, and the pair list's region of the fused
workspace (csrc/fused_layout.h)."""
import os
import subprocess

from amd import ROOT


def _run(tmp_path, name, flags=()):
    exe = tmp_path / name
    subprocess.run(["g++", "-O1", "-std=c++17", *flags, "-o", str(exe), os.path.join(ROOT, "tests", name + ".cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout


def test_pair_merge_against_sort(tmp_path):
    # the running top three with the tiles of the first two, and the merge of a
    # row's two lane halves, exhaustively over tied small-integer scores; a
    # stand-alone program, so the sanitizers run on it as they are
    _run(tmp_path, "pair_merge_check", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def test_pair_list_layout(tmp_path):
    # the pair list: a region of its own in the fix buffer exactly for the
    # single-pass euclidean refinement, its counter inside the cleared ones
    _run(tmp_path, "pair_layout_check")
