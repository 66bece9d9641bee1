"""bench.py on the GPU at a small size: a plain run prints the headline line
alone (what --full adds is absent), --steps sets the timed steps, and
--dump-outputs writes the last timed step's arrays -- checked against the CPU
oracle on the same seeded rows (the inputs depend on the arguments alone)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import assert_dist

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, L, KF, W, K = 30011, 128, 5, 4, np.float32(0.4), 256      # N: odd, several blocks; the bench's own d, L, k, w, K
SEED_DATA, SEED_PARAMS = 0x5EED, 12345


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LSHKM_DIST")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), *argv], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_the_timed_steps_outputs(tmp_path):
    res = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(N * 1e3 / res["ms_per_step"], rel=1e-9)
    assert res["unit"] == "point hash+assign ops/s" and res["higher_is_better"] is True and res["dtype"]
    # what --full adds is not measured in a plain run
    for key in ("roofline", "c5", "normal_data", "cpu_baseline"):
        assert key not in res, key
    assert "exact_distances" not in res["exactness"]

    got = _load(str(tmp_path))
    assert sorted(got) == ["assign", "bucket", "dist", "rows", "tuples"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert np.array_equal(got["rows"], np.arange(N))           # N below the sample size: every row
    X = oracle.synth(SEED_DATA, N, D)
    V, t, r, _ = oracle.gen_lsh_euclid(SEED_PARAMS, L, KF, D, W)
    tu, _, bu = oracle.lsh_hash_euclid(X, V, t, W, r, N // 100)
    crow = (np.arange(K) * (N // K)).astype(np.int32)
    oa, od = oracle.lloyd_assign(X, X[crow].astype(np.float64), "euclidean", crow)
    assert np.array_equal(got["tuples"], tu) and np.array_equal(got["bucket"], bu)
    assert np.array_equal(got["assign"], oa)
    assert_dist(got["dist"], od, "certified")


def test_c5_plain_run_dumps_centers_and_recommendations(tmp_path):
    res = _bench("--workload", "c5", "--k", "64", "--recom-users", "16", "--steps", "2", "--warmup", "1",
                 "--dump-outputs", str(tmp_path))
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    for key in ("roofline", "recommend", "km_sums_exchange_ms", "cpu_baseline"):
        assert key not in res, key
    got = _load(str(tmp_path))
    assert sorted(got) == ["assign", "bucket", "centers", "counts", "dist", "recommend", "rows", "tuples"]
    assert got["centers"].shape == (64, D) and got["recommend"].shape == (16, 5)
    assert got["counts"].sum() == N and np.array_equal(np.bincount(got["assign"].astype(np.int64), minlength=64),
                                                       got["counts"])
