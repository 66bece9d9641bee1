"""The PAM medoid update off the GPU: the ABI declares and the library exports
the entry points, the C++ drop-in's pam_lloyds compiles against the reference's
headers, and the golden fixtures are what tools/gen_pam_golden.cpp writes."""
import glob
import inspect
import os
import subprocess

import numpy as np
import pytest

from amd import PKG, lshkm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = "/root/reference/lib"
HAVE_REF = os.path.exists(os.path.join(REF_LIB, "clustering_phases", "update.hpp"))
PAM_DIR = os.path.join(ROOT, "tests", "golden", "pam")


def test_pam_symbols_declared_and_exported():
    declared = lshkm.declared_symbols()
    for sym in ("lshkm_pam_update", "lshkm_pam_update_f64"):
        assert sym in declared, sym
        for lib in ("liblshkm.so", "liblshkm_test.so"):
            out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], capture_output=True, text=True,
                                 check=True).stdout
            assert f" T {sym}\n" in out, (lib, sym)


def test_pam_python_surface():
    assert list(inspect.signature(lshkm.pam_update).parameters) == ["ctx", "X", "assign", "K", "metric", "prev_rows",
                                                                     "C_old"]
    assert (lshkm.STAT_PAM_SCREENED, lshkm.STAT_PAM_EXACT) == (10, 11)
    with open(os.path.join(PKG, "cluster.py")) as f:
        src = f.read()
    assert 'update="kmeans"' in src and '"pam"' in src       # the default stays k-means


def test_pam_fixtures_well_formed():
    files = sorted(glob.glob(os.path.join(PAM_DIR, "*.npz")))
    assert len(files) >= 8
    seen = set()
    for f in files:
        assert os.path.getsize(f) <= 1 << 20, f
        g = np.load(f)
        N, d = g["x"].shape
        K = len(g["prev_rows"])
        assert N <= 2000 and d in (8, 16, 100) and K <= 12, f
        assert g["assign"].shape == (N,) and set(g["assign"]) == set(range(K)), f      # no empty cluster
        for sfx in ("", "2"):
            med = g["medoid_rows" + sfx]
            assert np.array_equal(g["assign"][med], np.arange(K)), f                   # a member of its cluster
            assert g["sums" + sfx].shape == (K,)
        assert int(g["swapped2"][0]) == 0 and np.array_equal(g["medoid_rows"], g["medoid_rows2"]), f
        seen.add((int(g["metric"][0]), bool((g["prev_rows"] < 0).all()), bool(np.isnan(g["sums"]).any())))
    assert {m for m, _, _ in seen} == {0, 1}                 # both metrics
    assert any(k for _, k, _ in seen)                        # "k_means_center" predecessors
    assert any(n for _, _, n in seen)                        # zero rows under cosine: NaN sums


@pytest.mark.skipif(not HAVE_REF, reason="reference headers absent")
def test_pam_shim_compiles_against_reference(tmp_path):
    src = tmp_path / "shim_pam.cpp"
    src.write_text(
        '#include "utils.hpp"\n'
        '#include "lsh_cube.hpp"\n'
        '#include "clustering_phases/assignment.hpp"\n'
        '#include "clustering_phases/update.hpp"\n'
        '#include "clustering_phases/initialization.hpp"\n'
        '#include "lshkm_compat.hpp"\n'
        "template bool lshkm_compat::pam_lloyds<double>(std::vector<CustVector<double>>&,\n"
        "    std::vector<CustVector<double>*>&, std::string);\n"
        "template bool lshkm_compat::pam_lloyds<float>(std::vector<CustVector<float>>&,\n"
        "    std::vector<CustVector<float>*>&, std::string);\n"
        "// the reference's own signature takes the same arguments\n"
        "bool (*ref_fn)(std::vector<CustVector<double>>&, std::vector<CustVector<double>*>&, std::string) =\n"
        "    &pam_lloyds<double>;\n"
        "bool (*our_fn)(std::vector<CustVector<double>>&, std::vector<CustVector<double>*>&, std::string) =\n"
        "    &lshkm_compat::pam_lloyds<double>;\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wno-unused-function", "-I", REF_LIB,
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    own = [ln for ln in r.stderr.splitlines() if "lshkm_compat.hpp:" in ln and ("warning" in ln or "error" in ln)]
    assert not own, own


@pytest.mark.skipif(not HAVE_REF, reason="reference sources absent")
def test_pam_fixtures_reproduce(tmp_path):
    exe = tmp_path / "gen_pam_golden"
    subprocess.run(["g++", "-std=c++11", "-O0", "-w", "-I", REF_LIB, "-o", str(exe),
                    os.path.join(ROOT, "tools", "gen_pam_golden.cpp"), os.path.join(REF_LIB, "utils.cpp"),
                    os.path.join(REF_LIB, "data_structures", "tweet.cpp")], check=True)
    out = tmp_path / "pam"
    out.mkdir()
    log = subprocess.run([str(exe), str(out)], capture_output=True, text=True, check=True).stdout
    assert "dist_sum" in log and "bits 0x" in log             # the winning sums are printed
    made = sorted(os.listdir(out))
    assert made == sorted(os.listdir(PAM_DIR))
    for name in made:
        with open(out / name, "rb") as a, open(os.path.join(PAM_DIR, name), "rb") as b:
            assert a.read() == b.read(), name
