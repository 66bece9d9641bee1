"""GPU parity of the fused pass's hash fix-up (csrc/fused_small.hip,
hash_fixup_kernel): the rows the hi-only kernel lists with an uncertified floor
or sign get their tuples / phi / buckets from the fix-up, and these must be the
oracle's bit for bit whatever the lanes' layout of a row is. Small shapes that
reach every path of the kernel: ragged lists, one and several blocks, a tuple
buffer of 4-byte alignment, the soft-x87 fallback through the LDS image, every
function of every row, the cosine form, and two calls in a row. And the three
hash paths against each other (the fused pass + its fix-up, the standalone MFMA
hash + its fix kernel, the fp64 kernel) on rows no certificate passes: out of
the f16 range, non-finite, and with |(x.v + t) / w| beyond the int range."""
import ctypes as C

import numpy as np
import pytest

import oracle
from amd import lshkm
from conftest import assert_dist

pytestmark = pytest.mark.gpu

D, W = 128, np.float32(0.4)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def to_dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a)).to(ctx.dev)


def _centroids(K):
    # not fp32 values (as after an update), independent of the rows hashed
    return oracle.synth(0xCE27, K, D).astype(np.float64) * 1.001


def _check_euclid(ctx, Xh, L, k, K, dist_mode, seed=12345, nb=41):
    """hash_assign on Xh against the oracle: tuples, phi, buckets, cluster IDs bit
    for bit, distances per the mode. Returns (rows fixed up, soft-x87 values)."""
    V, t, r, _ = lshkm.params_lsh_euclidean(seed, L, k, D, float(W))
    lsh = lshkm.LSH(ctx, "euclidean", D, k, L, nb, float(W), V=V, t=t, r=r)
    Ch = _centroids(K)
    ctx.reset_stats()
    tu, ph, bu, a, dist = lshkm.hash_assign(lsh, to_dev(ctx, Xh), to_dev(ctx, Ch), None, tuples=True, phi=True,
                                            bucket=True)
    ctx.sync()
    fixed, soft = ctx.stat(lshkm.STAT_HASH_FIX), ctx.stat(lshkm.STAT_HASH_EXACT)
    xt, xp, xb = oracle.lsh_hash_euclid(Xh, V, t, W, r, nb)
    assert np.array_equal(tu.cpu().numpy(), xt)
    assert np.array_equal(ph.cpu().numpy(), xp)
    assert np.array_equal(bu.cpu().numpy(), xb)
    oa, od = oracle.lloyd_assign(Xh, Ch, "euclidean", None)
    assert np.array_equal(a.cpu().numpy(), oa)
    assert_dist(dist.cpu().numpy(), od, dist_mode)
    return fixed, soft


def _near_boundary_points(V, t, w, n, rng):
    """Rows whose (v0.x + t)/w sits within ~1e-15 of an integer: forces the exact path."""
    d = V.shape[-1]
    v = V.reshape(-1, d)[0].astype(np.float64)
    rows = []
    for i in range(n):
        x = np.zeros(d, np.float32)
        target = float(rng.integers(-20, 20))
        x[0] = np.float32((target * w - t.reshape(-1)[0]) / v[0])
        res = (v[0] * np.float64(x[0]) + np.float64(t.reshape(-1)[0])) / w - target
        x[1] = np.float32(-res * w / v[1])
        res2 = (v[0] * np.float64(x[0]) + v[1] * np.float64(x[1]) + np.float64(t.reshape(-1)[0])) / w - target
        x[2] = np.float32(-res2 * w / v[2])
        rows.append(x)
    return np.stack(rows)


@pytest.mark.parametrize("N", [1, 31, 33, 4099])
def test_fixup_ragged_n(ctx, N, dist_mode):
    # one partial tile, a tile boundary, several blocks with a ragged last tile
    Xh = ctx.synth(0x5EED, N, D).cpu().numpy()
    fixed, _ = _check_euclid(ctx, Xh, 5, 4, 64, dist_mode)
    if N == 4099:
        assert fixed > 0


def test_fixup_k320(ctx, dist_mode):
    # Kpad > 256: the hi-only kernel's 512-centroid form feeds the list
    Xh = ctx.synth(0x5EED, 4099, D).cpu().numpy()
    fixed, _ = _check_euclid(ctx, Xh, 5, 4, 320, dist_mode)
    assert fixed > 0


def test_fixup_boundary_rows(ctx, dist_mode):
    # uncertifiable floors: the soft-x87 chain reads the LDS image in the
    # reference's dimension order through the lanes' permuted index
    N, L, k, seed = 2051, 1, 4, 99
    V, t, _, _ = lshkm.params_lsh_euclidean(seed, L, k, D, float(W))
    Xh = oracle.synth(0xB0B, N, D).copy()
    where = np.random.default_rng(1).choice(N, 256, replace=False)
    Xh[where] = _near_boundary_points(V, t, W, 256, np.random.default_rng(0))
    _, soft = _check_euclid(ctx, Xh, L, k, 64, dist_mode, seed=seed, nb=7)
    assert soft > 0


def test_fixup_every_function_flagged(ctx, dist_mode):
    # one coordinate of 2^16 fails the f16 range guard (2^15): every function of
    # every row is flagged, so every row is listed with all 20 mask bits
    N = 300
    Xh = oracle.synth(0xF1A6, N, D).copy()
    Xh[np.arange(N), np.arange(N) % D] = np.float32(2.0 ** 16)
    fixed, _ = _check_euclid(ctx, Xh, 5, 4, 64, dist_mode)
    assert fixed == N


def test_fixup_unaligned_tuples(ctx):
    # a tuple buffer that is only 4-B aligned: the 16-B table accesses must not assume more
    N, L, k, K, nb = 4099, 5, 4, 64, 41
    V, t, r, _ = lshkm.params_lsh_euclidean(12345, L, k, D, float(W))
    lsh = lshkm.LSH(ctx, "euclidean", D, k, L, nb, float(W), V=V, t=t, r=r)
    X = ctx.synth(0x5EED, N, D)
    torch = ctx.torch
    raw = torch.zeros((N * L * k + 4,), dtype=torch.int32, device=ctx.dev)
    tu = raw[1:1 + N * L * k].view(N, L, k)
    assert tu.data_ptr() % 16 == 4
    bu = torch.empty((N, L), dtype=torch.int32, device=ctx.dev)
    a = torch.empty((N,), dtype=torch.int32, device=ctx.dev)
    dist = torch.empty((N,), dtype=torch.float64, device=ctx.dev)
    Cc = to_dev(ctx, _centroids(K))
    p = lambda x: C.c_void_p(x.data_ptr())
    ctx.reset_stats()
    lshkm._ck(lshkm.lib().lshkm_hash_assign(lsh.h, p(X), N, p(Cc), K, None, p(tu), None, p(bu), p(a), p(dist)))
    ctx.sync()
    assert ctx.stat(lshkm.STAT_HASH_FIX) > 0
    xt, _, xb = oracle.lsh_hash_euclid(X.cpu().numpy(), V, t, W, r, nb)
    assert np.array_equal(tu.cpu().numpy(), xt)
    assert np.array_equal(bu.cpu().numpy(), xb)
    assert int(raw[0].item()) == 0 and int(raw[-3:].abs().sum().item()) == 0      # nothing written around it


def test_fixup_cosine(ctx, dist_mode):
    # the cosine form: signs instead of floors; a zero row's inner products are
    # exactly zero, so its signs come from the soft-x87 chain
    N, L, k, K = 2051, 5, 4, 64
    Xh = oracle.synth(0xC05, N, D).copy()
    Xh[7] = 0.0
    R, _ = lshkm.params_lsh_cosine(21, L, k, D)
    lsh = lshkm.LSH(ctx, "cosine", D, k, L, R=R)
    Ch = _centroids(K)
    ctx.reset_stats()
    _, ph, bu, a, dist = lshkm.hash_assign(lsh, to_dev(ctx, Xh), to_dev(ctx, Ch), phi=True, bucket=True,
                                           metric="cosine")
    ctx.sync()
    assert ctx.stat(lshkm.STAT_HASH_EXACT) >= 1
    og = oracle.lsh_hash_cosine(Xh, R.reshape(L, k, D))
    assert np.array_equal(bu.cpu().numpy(), og)
    assert np.array_equal(ph.cpu().numpy(), og)
    oa, od = oracle.lloyd_assign(Xh, Ch, "cosine", None)
    assert np.array_equal(a.cpu().numpy(), oa)
    assert np.array_equal(dist.cpu().numpy().view(np.uint64), od.view(np.uint64))


def test_fixup_repeat_call(ctx, dist_mode):
    # two calls in a row on one context with different rows: no list, LDS or
    # stream state may carry over
    for seed, N in ((0xA1, 4099), (0xA2, 3001), (0xA1, 4099)):
        Xh = oracle.synth(seed, N, D)
        fixed, _ = _check_euclid(ctx, Xh, 5, 4, 64, dist_mode)
        assert fixed > 0


# ---- the three hash paths on the rows that defeat every certificate -------------
SP_N, SP_K, SP_W = 2048 + 17, 64, 0.01


@pytest.fixture(scope="module")
def special_rows():
    from test_gpu_hash_mfma import rows
    X = rows(SP_N, 77)            # zero, 1e-30, x4e4, inf, NaN, subnormal, 3e38, tied grids
    X[700:720] *= np.float32(3e7)  # |(x.v + t) / w| >= 2^31 at w = 0.01, both signs: the reference stores INT_MIN
    X[720:740] *= np.float32(2e6)  # ... and around 2^31
    return np.ascontiguousarray(X, np.float32)


def _same(got, want, what, rows=None):
    for name, u, v in zip(("tuples", "phi", "bucket"), got, want):
        assert (u is None) == (v is None), (what, name)
        if u is None:
            continue
        if rows is not None:
            u = u[rows]
        bad = np.nonzero((u != v).reshape(len(u), -1).any(axis=1))[0]
        assert bad.size == 0, (what, name, (bad if rows is None else rows[bad])[:20])


def _host(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("metric,L,k,form", [("euclidean", 5, 4, "persistent"), ("cosine", 5, 4, "persistent"),
                                             ("euclidean", 3, 7, "chunked")])
def test_hash_paths_agree_on_special_rows(ctx, sctx, sw, special_rows, monkeypatch, metric, L, k, form):
    from test_gpu_hash_mfma import fp64_path
    Xh = special_rows
    X = to_dev(ctx, Xh)
    Cd = to_dev(ctx, _centroids(SP_K))
    nb = 41
    if metric == "euclidean":
        V, t, r, _ = lshkm.params_lsh_euclidean(123, L, k, D, SP_W)
        mk = lambda M, c: M.LSH(c, metric, D, k, L, nb, SP_W, V=V, t=t, r=r)
    else:
        R, _ = lshkm.params_lsh_cosine(123, L, k, D)
        mk = lambda M, c: M.LSH(c, metric, D, k, L, R=R)
    # the fused pass (chunked: the streaming form, forced in the test build) + its fix-up
    M, c = (lshkm, ctx) if form == "persistent" else (sw, sctx)
    if form == "chunked":
        monkeypatch.setenv("LSHKM_FUSED_FORM", "chunked")
    fused = _host(M.hash_assign(mk(M, c), X, Cd, None, tuples=True, phi=True, bucket=True,
                                metric=None if metric == "euclidean" else "cosine")[:3])
    c.sync()
    # the standalone MFMA hash + its fix kernel, and the fp64 kernel
    mfma = _host(mk(lshkm, ctx).hash(X))
    with fp64_path():
        fp64 = _host(mk(sw, sctx).hash(X))
    _same(fused, fp64, "fused pass vs fp64 kernel")
    _same(mfma, fp64, "MFMA hash vs fp64 kernel")
    fin = np.nonzero(np.isfinite(Xh).all(axis=1))[0]
    if metric == "euclidean":
        want = oracle.lsh_hash_euclid(Xh[fin], V, t, np.float32(SP_W), r, nb)
        assert (want[0][np.isin(fin, np.arange(700, 720))] == np.int32(-2 ** 31)).any()   # the rows do leave the int range
    else:
        og = oracle.lsh_hash_cosine(Xh[fin], R.reshape(L, k, D))
        want = (None, og, og)
    _same(fused, want, "fused pass vs oracle", fin)
    _same(mfma, want, "MFMA hash vs oracle", fin)
