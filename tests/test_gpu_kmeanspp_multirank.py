"""Sharded k-means++ seeding over real ranks: two fresh processes
share the one MI355X over gloo, each running lshkm.KppShard on its row shard
under sharding.kmeans_pp_sharded (tests/kpp_worker.py), against one process
over all rows and the CPU oracle: the chosen rows and C0 on every rank, and one
ShardedLloyd.step() from that seeding (cluster IDs and centers). At most three
processes hold the GPU: the suite's own and the two ranks (the single-process
run ends before they start)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "kpp_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, out):
    port = str(_free_port())
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    procs = [subprocess.Popen([sys.executable, "-u", WORKER, str(r), str(world), port, str(out)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=180)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    return [dict(np.load(os.path.join(out, f"rank{r}.npz"))) for r in range(world)]


def test_two_ranks_on_one_gpu_match_single_process_and_oracle(tmp_path):
    (tmp_path / "one").mkdir()
    (tmp_path / "two").mkdir()
    one = _run(1, tmp_path / "one")[0]          # a failed rank raises here: nothing starts after it
    two = _run(2, tmp_path / "two")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kpp_worker
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for leg, (dseed, N, d, K, metric, seed) in kpp_worker.LEGS.items():
        X = oracle.synth(dseed, N, d)
        want = oracle.kmeans_pp(X, K, metric, seed)
        for r in [one] + two:
            assert np.array_equal(r[f"{leg}_rows"], want), leg
            assert np.array_equal(bits(r[f"{leg}_C0"]), bits(X[want].astype(np.float64))), leg
        # one Lloyd + k-means step from that seeding: IDs per row, the same centers on every rank
        assert np.array_equal(np.concatenate([r[f"{leg}_assign"] for r in two]), one[f"{leg}_assign"]), leg
        for r in two:
            assert np.array_equal(bits(r[f"{leg}_centers"]), bits(one[f"{leg}_centers"])), leg
