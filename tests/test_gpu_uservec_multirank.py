"""clusters_to_user_vectors over real ranks: three fresh processes share the one
MI355X over gloo, each holding a contiguous third of the `mid` fixture's
clustered rows (tests/uservec_worker.py); the (sum, known) carry goes rank to
rank and every rank finishes the totals. Every rank's bundle equals the list
the reference's own function produced (tests/golden/uservec/mid.npz), bit for
bit. Four processes hold the GPU at most: the suite's own and the three ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from uservec_np import bits, load, strs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "uservec_worker.py")


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


def test_three_ranks_on_one_gpu_match_the_reference(tmp_path):
    g = load("mid")
    for r in _run(3, tmp_path):
        assert [str(i) for i in r["ids"]] == strs(g, "b_id") and np.array_equal(r["src"], r["ids"])
        assert np.array_equal(bits(r["x"]), bits(g["b_x"])) and np.array_equal(bits(r["mean"]), bits(g["b_mean"]))
        assert np.array_equal(r["unk_ptr"], g["b_unk_ptr"]) and np.array_equal(r["unk_idx"], g["b_unk_idx"])
