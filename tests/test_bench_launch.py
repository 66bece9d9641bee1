"""bench.py's multi-rank launch on CPU: `--gpus N` starts N ranks itself (under
torch.distributed.run, before any GPU call), each rank sees WORLD_SIZE = N, and
the C5 exchange (sharding.allreduce_partials) and the max-over-ranks timing run
over gloo (--dry-run: no GPU work)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]          # rank 0 alone prints
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_bench_spawns_ranks(n):
    res = _bench("--gpus", str(n), "--dry-run", "--full", "--steps", "2", "--warmup", "1", "--n", "1000", "--k", "64",
                 "--cpu-hash-sample", "2000", "--cpu-assign-sample", "400", "--cpu-port-hash-sample", "2000",
                 "--cpu-port-assign-sample", "400")
    assert res["dry_run"] and res["n_gpus"] == n and res["world_size"] == n and res["backend"] == "gloo"
    # rank 0 times the reference's CPU path in the same run at every N (after the final barrier)
    cb = res["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("reference", "port"), cb
    assert "all_cores" in cb
    assert res["allreduce_ok"]
    assert [s["rank"] for s in res["shards"]] == list(range(n))
    assert sum(s["n"] for s in res["shards"]) == 1000 * n
    assert res["ms_per_step"] > 0


def test_plain_run_leaves_out_what_full_adds():
    res = _bench("--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1", "--n", "1000", "--k", "64")
    assert res["dry_run"] and res["steps"] == 3 and res["ms_per_step"] > 0
    assert "cpu_baseline" not in res


def test_dump_outputs_samples_fixed_rows(tmp_path):
    # per-row arrays beyond DUMP_ROWS rows: a sorted, seeded sample without repeats,
    # the same on every call; small arrays whole; everything float64
    import importlib.util

    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("lshkm_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.DUMP_ROWS + 7
    per_row = {"a": torch.arange(n, dtype=torch.int32), "b": torch.arange(2 * n, dtype=torch.float64).reshape(n, 2)}
    for sub in ("x", "y"):
        bench.dump_outputs(str(tmp_path / sub), 0, 1, per_row, {"w": torch.ones(3, dtype=torch.int64)})
    got = {f[:-4]: np.load(tmp_path / "x" / f) for f in sorted(os.listdir(tmp_path / "x"))}
    assert sorted(got) == ["a", "b", "rows", "w"] and all(v.dtype == np.float64 for v in got.values())
    rows = got["rows"]
    assert rows.shape == (bench.DUMP_ROWS,) and np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < n
    assert np.array_equal(got["a"], rows) and np.array_equal(got["b"][:, 0], 2 * rows) and got["w"].tolist() == [1, 1, 1]
    # the C5 dump, the larger one: tuples, bucket IDs, cluster ID, distance and row index per sampled row,
    # 1024 centers and counts, 1024 users' top 5 -- within the 64 MB a dump may take
    per_sampled_row = bench.L_TABLES * bench.K_FUNCS + bench.L_TABLES + 3
    assert 8 * (bench.DUMP_ROWS * per_sampled_row + 1024 * (bench.D + 1) + 1024 * 5) <= 64 << 20
    for name, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "y" / (name + ".npy"))), name
    # at N > 1 every rank writes files of its own
    bench.dump_outputs(str(tmp_path / "z"), 1, 2, {"a": torch.arange(5)}, {})
    assert sorted(os.listdir(tmp_path / "z")) == ["a.rank1.npy", "rows.rank1.npy"]


def test_bench_rejects_mismatched_world():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--dry-run"], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "WORLD_SIZE=2" in out.stderr
