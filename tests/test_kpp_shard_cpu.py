"""Sharded k-means++ seeding on the CPU: the protocol of
sharding.kmeans_pp_sharded (k_means_pp, initialization.hpp:71-156, over
contiguous row shards) with the numpy restatement of the per-rank calls
(tests/kpp_shard_np.py) against oracle.kmeans_pp on the concatenated rows --
over the in-process exchange and over gloo ranks -- and the library's host-only
draws (lshkm_kpp_draws). The GPU library's calls: tests/test_gpu_kmeanspp_shard.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _imports():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle
    from amd import PKG, lshkm
    sys.path.insert(0, PKG)
    import sharding as sh
    from kpp_shard_np import NumpyKppShard
    return oracle, lshkm, sh, NumpyKppShard


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case(oracle, name):
    """(X, K, metric, seed) of a named case."""
    if name == "euclid":
        return oracle.synth(0x5EED ^ 21, 3001, 8), 9, "euclidean", 31
    if name == "cosine_zero":
        X = oracle.synth(0x5EED ^ 22, 2000, 16)
        X[[7, 1203]] = 0.0                                   # two all-zero rows: NaN cosine distances
        return X, 6, "cosine", 32
    if name == "repeated":
        N = 2400
        return oracle.synth(0x5EED ^ 23, N, 8)[np.arange(N) // 3], 7, "euclidean", 33
    if name == "equal":
        return np.ones((1000, 8), np.float32), 5, "euclidean", 3    # max 0: a NaN total, so row 0
    assert name == "one_row"
    return oracle.synth(5, 1, 16), 3, "euclidean", 9


CASES = ["euclid", "cosine_zero", "repeated", "equal", "one_row"]


@pytest.mark.parametrize("seed,N", [(1, 1), (2, 7), (31, 3001), (77, 100_000), (12345, 2_000_000)])
def test_kpp_draws_first_row_matches_oracle(seed, N):
    oracle, lshkm, _, _ = _imports()
    first, canon = lshkm.kpp_draws(seed, N, 4)
    assert first == oracle.kmeans_pp(np.zeros((N, 1), np.float32), 1, "euclidean", seed)[0]
    assert canon[0] == 0.0 and ((canon[1:] >= 0.0) & (canon[1:] < 1.0)).all()
    # the draws of a shorter run are a prefix: the engine is consumed in the reference's order
    assert np.array_equal(lshkm.kpp_draws(seed, N, 3)[1], canon[:3])


@pytest.mark.parametrize("name,world", [(c, w) for c in CASES[:4] for w in (1, 2, 3, 5)] + [("one_row", 2)])
def test_in_process_shards_match_oracle(name, world):
    oracle, lshkm, sh, NumpyKppShard = _imports()
    X, K, metric, seed = _case(oracle, name)
    N = X.shape[0]
    spans = [sh.shard_range(N, world, r) for r in range(world)]
    ops = [NumpyKppShard(X[a:a + n], metric) for a, n in spans]
    rows, C0 = sh.kmeans_pp_sharded(ops, [a for a, _ in spans], [n for _, n in spans], N, K, seed,
                                    exchange=sh.LocalExchange())
    want = oracle.kmeans_pp(X, K, metric, seed)
    assert np.array_equal(rows, want)
    assert np.array_equal(C0.view(np.uint64), X[want].astype(np.float64).view(np.uint64))
    if name == "equal":
        assert (rows[1:] == 0).all()
    if name == "one_row":
        assert spans[1][1] == 0                              # an empty shard took part


def _gloo_worker(rank, world, port, name, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    oracle, lshkm, sh, NumpyKppShard = _imports()
    X, K, metric, seed = _case(oracle, name)
    N = X.shape[0]
    row0, n = sh.shard_range(N, world, rank)
    rows, C0 = sh.kmeans_pp_sharded(NumpyKppShard(X[row0:row0 + n], metric), row0, n, N, K, seed)
    np.savez(out_path + f".{rank}.npz", rows=rows, C0=C0)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["euclid", "cosine_zero", "equal"])
def test_gloo_ranks_match_oracle(name, world, tmp_path):
    out = str(tmp_path / "kpp")
    mp.spawn(_gloo_worker, args=(world, _free_port(), name, out), nprocs=world, join=True)
    oracle, _, _, _ = _imports()
    X, K, metric, seed = _case(oracle, name)
    want = oracle.kmeans_pp(X, K, metric, seed)
    for r in range(world):                                   # every rank: the same rows and the same C0
        got = np.load(out + f".{r}.npz")
        assert np.array_equal(got["rows"], want), r
        assert np.array_equal(got["C0"].view(np.uint64), X[want].astype(np.float64).view(np.uint64)), r


def test_gloo_empty_shard(tmp_path):
    # N = 1 over two ranks: rank 1 holds no row
    out = str(tmp_path / "kpp1")
    mp.spawn(_gloo_worker, args=(2, _free_port(), "one_row", out), nprocs=2, join=True)
    oracle, _, _, _ = _imports()
    X, K, metric, seed = _case(oracle, "one_row")
    for r in range(2):
        assert np.array_equal(np.load(out + f".{r}.npz")["rows"], oracle.kmeans_pp(X, K, metric, seed))
