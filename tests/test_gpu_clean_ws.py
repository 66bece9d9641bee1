"""The fused assignment's clean workspace (csrc/fused.hip): a call's last kernel
leaves its counters and the centroid prep's bound words zeroed and the context
records that, so the next fused call clears nothing; every other user of the two
buffers and a reallocation drop the record. One context takes fused calls
interleaved with an f32-MFMA assignment (d = 200: the one other user of the two
buffers, which must drop the record), range assignments (leftover rows through
the fused pass at d = 128, through the f32-MFMA kernel at d = 200), a call that
fails its argument check (refused before the fused pass starts: the record
must survive it unharmed) and shapes that reallocate; every call's outputs and
per-call counters must equal a fresh context's. The epilogue's centroid
override is checked against the oracle at centroid counts on both sides of its
LDS form's limit."""
import ctypes as C

import numpy as np
import pytest

import oracle
from amd import lshkm
from conftest import assert_dist

pytestmark = pytest.mark.gpu

N_STATS = 17
GRID = np.arange(-4, 5) * 0.5


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def dataset(seed, N, K, d, dtype=np.float32):
    """Grid centroids; rows: exact midpoints of centroid pairs (never certified),
    three-way ties, copies of centroids."""
    rng = np.random.default_rng(seed)
    Cc = np.unique(rng.choice(GRID, size=(4 * K + 16, d)), axis=0)
    Cc = Cc[rng.permutation(len(Cc))[:K]].astype(np.float64)
    base = rng.choice(GRID, size=d)
    for i, c in enumerate([1, K // 2, K - 1]):
        Cc[c] = base
        Cc[c][i] += 1.0
    mids = (Cc[rng.integers(0, K, 20)] + Cc[rng.integers(0, K, 20)]) / 2
    X = np.concatenate([mids, [base], Cc[rng.integers(0, K, N)]])[:N].astype(dtype)
    src = rng.integers(0, N, K).astype(np.int32)
    return X, Cc, src


def test_interleaved_calls_match_fresh_contexts(ctx):
    torch = ctx.torch
    A = dataset(1, 1000, 64, 128)
    B = dataset(2, 4000, 256, 128)          # more rows and centroids than A: the buffers grow
    G = dataset(3, 900, 40, 100, np.float64)
    M = dataset(4, 800, 32, 200)            # 128 < d <= 256: the f32-MFMA path (fewer centroids than A: no reallocation)
    V, t, r, _ = lshkm.params_lsh_euclidean(77, 5, 4, 128, 0.4)

    def dev(c, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(c.dev)

    def fused(data, metric="euclidean", src=True):
        X, Cc, sr = data
        return lambda c: lshkm.lloyd_assign(c, dev(c, X), dev(c, Cc), metric, sr if src else None)

    def hashed(data):
        X, Cc, sr = data
        return lambda c: lshkm.hash_assign(lshkm.LSH(c, "euclidean", 128, 4, 5, 97, 0.4, V=V, t=t, r=r), dev(c, X),
                                           dev(c, Cc), sr)

    def ranged(data):
        X, Cc, sr = data
        K, N = len(Cc), len(X)
        rng = np.random.default_rng(9)
        ptr = np.arange(K + 1, dtype=np.int64) * 5
        idx = rng.integers(0, N, 5 * K).astype(np.int32)
        return lambda c: lshkm.range_assign(c, dev(c, X), dev(c, Cc), ptr, idx, "euclidean", src_rows=sr)[:2]

    def exact_mode(call):
        def run(c):
            c.set_dist_mode("exact")
            try:
                return call(c)
            finally:
                c.set_dist_mode("certified")
        return run

    def bad_metric(c):
        X, Cc, _ = A
        Xd, Cd = dev(c, X), dev(c, Cc)
        a, dd = c.empty((len(X),), torch.int32), c.empty((len(X),), torch.float64)
        rc = lshkm.lib().lshkm_lloyd_assign(c.h, C.c_void_p(Xd.data_ptr()), C.c_int64(len(X)), 128,
                                            C.c_void_p(Cd.data_ptr()), len(Cc), 99, None, C.c_void_p(a.data_ptr()),
                                            C.c_void_p(dd.data_ptr()))
        assert rc != 0
        return ()

    calls = [("A", fused(A)), ("A again", fused(A)), ("f32-MFMA", fused(M)), ("A after f32-MFMA", fused(A)),
             ("range", ranged(A)), ("A after range", fused(A)), ("range d=200", ranged(M)),
             ("A after range d=200", fused(A)), ("bad metric", bad_metric),
             ("A after the failed call", fused(A, src=False)), ("B: reallocation", fused(B)), ("A after B", fused(A)),
             ("hashed", hashed(A)), ("A after hashed", fused(A)), ("cosine", fused(A, "cosine")),
             ("A after cosine", fused(A)), ("exact mode", exact_mode(fused(A))), ("A after exact", fused(A)),
             ("fp64 rows", fused(G)), ("A after fp64", fused(A)), ("hashed B", hashed(B)), ("B", fused(B))]

    def run(c, call):
        c.reset_stats()
        out = call(c)
        c.sync()
        return [o.cpu().numpy() for o in out if o is not None], [c.stat(i) for i in range(N_STATS)]

    for name, call in calls:
        got, st = run(ctx, call)
        want, st0 = run(lshkm.Context(0), call)
        assert st == st0, name
        # the path each call took: the fused pass refines the midpoints it cannot
        # certify at once, the f32-MFMA kernel lists them without a refinement
        if name == "f32-MFMA":
            assert st[lshkm.STAT_REFINED] == 0 and st[lshkm.STAT_ASSIGN_AMBIG] > 0, st
        elif name.startswith("A"):
            assert st[lshkm.STAT_REFINED] > 0 and st[lshkm.STAT_ASSIGN_AMBIG] > 0, (name, st)
        assert len(got) == len(want)
        for u, v in zip(got, want):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), name


@pytest.mark.parametrize("K", [3000, 8192, 8200])
def test_override_at_large_k(ctx, dist_mode, K):
    # fp32 rows of d = 128 take the fused pass at any K; its epilogue applies the
    # override in LDS up to 8192 centroids (a block of 1024 threads here) and by
    # the override's global-memory kernel past that. Many centroids name one row:
    # the last one wins.
    torch = ctx.torch
    rng = np.random.default_rng(K)
    N, d = 200, 128
    Cc = rng.choice(GRID, size=(K, d)).astype(np.float64)
    X = np.concatenate([Cc[rng.integers(0, K, N - 4)], (Cc[:4] + Cc[4:8]) / 2]).astype(np.float32)
    src = np.full(K, -1, np.int32)                     # -1: no source row
    src[rng.choice(K, 150, replace=False)] = rng.integers(0, N // 2, 150)     # the upper half keeps the pass's results
    src[-3:] = [5, N - 1, 5]
    Xd, Cd = torch.from_numpy(X).to(ctx.dev), torch.from_numpy(Cc).to(ctx.dev)
    oa, od = oracle.lloyd_assign(X, Cc, "euclidean", src)
    for _ in range(2):                                  # the second call: a clean workspace
        a, dist = lshkm.lloyd_assign(ctx, Xd, Cd, "euclidean", src)
        ctx.sync()
        assert np.array_equal(a.cpu().numpy(), oa)
        assert_dist(dist.cpu().numpy(), od, dist_mode)
    assert oa[5] == K - 1 and oa[N - 1] == K - 2
