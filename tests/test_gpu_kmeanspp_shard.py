"""GPU parity: k-means++ seeding over row shards (lshkm_kpp_shard_*,
sharding.kmeans_pp_sharded; k_means_pp, initialization.hpp:71-156) -- the
chosen rows, bit-exact -- with every shard in this process on one context
(sharding.LocalExchange): against the reference's golden outputs under several
shard layouts, against the CPU oracle and the single-device entry
(lshkm_kmeans_pp) at sizes and inputs the golden cases do not reach, with a
shard boundary placed on a binade crossing of the prefix sums, and with the
walk's counters (a shard's walk stays an integer walk)."""
import sys

import numpy as np
import pytest

import oracle
from amd import PKG, lshkm
from conftest import cases, golden, golden_meta, kpp_input
from kpp_shard_np import NumpyKppShard

sys.path.insert(0, PKG)
import sharding as sh  # noqa: E402

META = golden_meta()
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def to_dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a)).to(ctx.dev)


def sharded(ctx, X, cuts, K, metric, seed):
    """kmeans_pp_sharded over the row shards [cuts[i], cuts[i + 1]) of X."""
    cuts = [int(c) for c in cuts]
    assert cuts[0] == 0 and cuts[-1] == X.shape[0]
    ops = [lshkm.KppShard(ctx, to_dev(ctx, X[a:b]), metric) for a, b in zip(cuts, cuts[1:])]
    rows, C0 = sh.kmeans_pp_sharded(ops, cuts[:-1], [b - a for a, b in zip(cuts, cuts[1:])], X.shape[0], K, seed,
                                    exchange=sh.LocalExchange())
    assert np.array_equal(C0.view(np.uint64), X[rows].astype(np.float64).view(np.uint64))
    return rows


def equal_cuts(N, world):
    return [sh.shard_range(N, world, r)[0] for r in range(world)] + [N]


SPLITS = {
    "eq1": lambda N: equal_cuts(N, 1),
    "eq2": lambda N: equal_cuts(N, 2),
    "eq3": lambda N: equal_cuts(N, 3),
    "ragged": lambda N: [0, N // 3 + 37, 2 * N // 3 + 101, N],        # multiples of neither 256 nor 512
    "small": lambda N: [0, N // 2 + 3, N // 2 + 44, N],               # a shard of 41 rows
    "empty": lambda N: [0, N // 2 + 5, N // 2 + 5, N],                # an empty shard in the middle
}


@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("name", cases("kmeanspp"))
def test_sharded_kmeans_pp_golden(ctx, name, split):
    m, g = META[name], golden(name)
    cuts = SPLITS[split](m["N"])
    if split == "ragged":
        assert all(c % 256 for c in cuts[1:-1])
    rows = sharded(ctx, kpp_input(name), cuts, m["K"], m["metric"], m["seed"])
    assert np.array_equal(rows, g["kpp_rows"])


def _general64(seed, N, d):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, d)) * np.exp(rng.uniform(-2, 2, size=(N, 1)))


def _cos_zero(N, d):
    X = oracle.synth(141, N, d)
    X[[0, 5, N // 2, N - 1]] = 0.0          # all-zero rows: NaN cosine distances, a NaN total
    return X


ORACLE_CASES = {
    # name: (rows, K, metric, seed, cuts)
    "e16": (lambda: oracle.synth(131, 20_000, 16), 12, "euclidean", 41, [0, 700, 701, 9473, 20_000]),
    "e128": (lambda: oracle.synth(132, 6_000, 128), 6, "euclidean", 42, [0, 1999, 4100, 6_000]),   # kpp_dist_reg_kernel
    "c128": (lambda: oracle.synth(133, 6_000, 128), 6, "cosine", 43, [0, 1999, 4100, 6_000]),      # the VEC cosine form
    "f64_e16": (lambda: _general64(51, 20_000, 16), 12, "euclidean", 44, [0, 700, 701, 9473, 20_000]),
    "f64_e128": (lambda: _general64(52, 6_000, 128), 6, "euclidean", 45, [0, 1999, 4100, 6_000]),
    "f64_c128": (lambda: _general64(53, 6_000, 128), 6, "cosine", 46, [0, 1999, 4100, 6_000]),
    "repeated": (lambda: oracle.synth(134, 9_000, 16)[np.arange(9_000) // 3], 8, "euclidean", 47, [0, 2999, 6001, 9_000]),
    "equal": (lambda: np.ones((3_000, 8), np.float32), 5, "euclidean", 3, [0, 1000, 2100, 3_000]),
    "cos_zero": (lambda: _cos_zero(4_000, 16), 6, "cosine", 48, [0, 1300, 2000, 4_000]),
    "one_row": (lambda: oracle.synth(5, 1, 16), 3, "euclidean", 9, [0, 1, 1]),
    "k40": (lambda: oracle.synth(115, 777, 5), 40, "euclidean", 15, equal_cuts(777, 3)),
}


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_sharded_kmeans_pp_matches_oracle_and_single_device(ctx, name):
    make, K, metric, seed, cuts = ORACLE_CASES[name]
    X = make()
    want = oracle.kmeans_pp(X, K, metric, seed)
    one = lshkm.kmeans_pp_rows(ctx, to_dev(ctx, X), K, metric, seed)
    got = sharded(ctx, X, cuts, K, metric, seed)
    assert np.array_equal(one, want)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("K", [2, 3])
def test_binade_crossing_on_a_shard_boundary(ctx, K):
    N, d, metric, seed = 6_000, 16, "euclidean", 61
    X = oracle.synth(135, N, d)
    # iteration 1's prefix sums on the CPU
    first, _ = lshkm.kpp_draws(seed, N, K)
    ref = NumpyKppShard(X, metric)
    mb, _ = ref.dist(X[first].astype(np.float64), 1)
    ref.units(mb, 0.0)
    ref.chain(0.0)
    e = np.frexp(ref.cum)[1]
    m = next(i for i in range(513, N) if e[i] > e[i - 1])    # row m's sum lies in a higher binade than row m - 1's
    assert m + 1 < N
    got = sharded(ctx, X, [0, m, m + 1, N], K, metric, seed)  # one shard starts at the crossing row, one right after it
    assert np.array_equal(got, oracle.kmeans_pp(X, K, metric, seed))


def test_shard_walk_stays_an_integer_walk(ctx):
    N, d, K, metric, seed = 300_000, 16, 6, "euclidean", 11
    X = oracle.synth(seed + 100, N, d)
    cuts = equal_cuts(N, 2)
    ctx.reset_stats()
    got = sharded(ctx, X, cuts, K, metric, seed)
    chunks, seq = ctx.stat(2), ctx.stat(3)
    assert np.array_equal(got, oracle.kmeans_pp(X, K, metric, seed))
    print(f"chunks {chunks} sequential {seq}")
    assert chunks == (K - 1) * sum((b - a + 511) // 512 for a, b in zip(cuts, cuts[1:]))
    # the bound tests/test_gpu_kmeanspp.py holds the single-device walk to at this
    # size: with s_in > 0 the second shard's first chunk is an integer chunk too
    assert seq <= (K - 1) * 40, (seq, chunks)
