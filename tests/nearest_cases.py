"""Fixtures of tests/golden/nearest (tools/gen_nearest_golden.cpp), shared by
tests/test_nearest_cpu.py and tests/test_gpu_nearest.py."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "nearest")
FIXTURES = sorted(f[:-4] for f in os.listdir(DIR) if f.endswith(".npz"))


def fixture(name):
    """(x [N][d] f64, q [nq][d] f64, metric name, dist [nq] f64: the reference's)."""
    g = np.load(os.path.join(DIR, name + ".npz"))
    return g["x"], g["q"], "cosine" if int(g["metric"][0]) else "euclidean", g["dist"]


def fixture_is_f32(name):
    return bool(np.load(os.path.join(DIR, name + ".npz"))["f32"][0])


def first_row(x, q, metric, dist):
    """The first row attaining each query's reference distance (-1: N == 0; row 0
    for a NaN, which only row 0 can give): the oracle's argmin, whose loop
    replaces on strict < alone (tests/test_nearest_cpu.py pins its values to the
    fixture's)."""
    import oracle
    if x.shape[0] == 0:
        return np.full(q.shape[0], -1, np.int32)
    a, od = oracle.lloyd_assign(q, x, metric)
    assert np.array_equal(od.view(np.uint64), dist.view(np.uint64))
    return a
