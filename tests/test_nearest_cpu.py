"""lshkm_min_vector_dist without a GPU.

1. Every fixture of tests/golden/nearest (tools/gen_nearest_golden.cpp: the
   reference's own min_vector_euclidean_dist / min_vector_cosine_dist) equals
   oracle.lloyd_assign(q, x, metric)[1] bit for bit (N >= 1). The two loops
   differ only in the oracle's -1 sentinel, which no distance can equal; this
   pins the oracle as the expectation of the larger cases of
   tests/test_gpu_nearest.py.
2. csrc/nearest_layout.h's route, capacity, segment and workspace arithmetic at
   its edges, through tests/nearest_layout_check.cpp."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from nearest_cases import FIXTURES, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_set():
    """Both metrics of every case the generator writes."""
    names = {n.split("_", 1)[1] for n in FIXTURES}
    assert names == {"general", "f32", "dyadic", "dup", "zero0", "zero_mid", "inf0", "inf_mid", "big", "n1", "n0"}
    assert len(FIXTURES) == 2 * len(names)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference(name):
    x, q, metric, dist = fixture(name)
    assert dist.shape == (q.shape[0],) and x.shape[0] <= 600 and q.shape[0] <= 64
    if x.shape[0] == 0:
        assert np.array_equal(dist.view(np.uint64), np.zeros(q.shape[0], np.uint64))     # utils.hpp:109-110
        return
    _, od = oracle.lloyd_assign(q, x, metric)
    assert np.array_equal(od.view(np.uint64), dist.view(np.uint64)), np.nonzero(od.view(np.uint64) != dist.view(np.uint64))


def test_fixtures_hold_their_edges():
    """What each hard case is there for is present in its data and result."""
    for m in ("eu", "cos"):
        x, q, _, dist = fixture(f"{m}_dup")
        assert np.array_equal(x[0::2], x[1::2])
        x, q, _, dist = fixture(f"{m}_inf0")
        assert np.isinf(x[0]).any() and np.isinf(q[-1]).any()
        x, q, _, dist = fixture(f"{m}_inf_mid")
        assert np.isinf(x[x.shape[0] // 2]).any() and not np.isinf(x[0]).any()
        x, q, _, dist = fixture(f"{m}_big")
        assert (np.abs(x) == 1e200).any() and (np.abs(x) == 1e-200).any() and (np.abs(q) == 1e200).any()
    x, q, _, dist = fixture("cos_zero0")
    assert not x[0].any() and np.isnan(dist).all(), "a zero row 0 under cosine: every query's result is its NaN"
    x, q, _, dist = fixture("cos_zero_mid")
    assert not x[x.shape[0] // 2].any() and np.isfinite(dist[:-1]).all() and np.isnan(dist[-1])
    x, q, _, dist = fixture("eu_inf0")
    assert np.isnan(dist[-1]) and np.isfinite(dist[:-2]).all(), "inf - inf at row 0 is the answer; else inf loses"
    x, q, _, dist = fixture("eu_dyadic")
    _, od = oracle.lloyd_assign(q, x, "euclidean")
    ties = sum(int((np.sqrt(((x - qq) ** 2).sum(1)) == dd).sum() > 1) for qq, dd in zip(q, od))
    assert ties >= q.shape[0] // 2, "the dyadic case holds exact ties for most queries"


def test_nearest_layout(tmp_path):
    exe = tmp_path / "nearest_layout_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "nearest_layout_check.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
