"""GPU: the hi-only FAST pass with its rows fetched one tile ahead.

fused_hi_kernel<.., FAST, PF> (K <= 256, euclidean, certified mode, fp32 rows of
128 dims) takes dims 0..63 of a wave's next tile through an LDS-DMA buffer and
dims 64..127 through registers the centroid loop left dead. The checks use paths
that do not contain that code: the standalone MFMA hash (LSH.hash), the exact
mode (the gather-ring kernels), the CPU oracle, and the test build's
LSHKM_ROW_PREFETCH=0 (the same kernel with its rows loaded at the tile's top),
which must give identical outputs and counters.

Row counts: a single tile and its edges; and, with cu compute units of 8 waves
of 32-row tiles, cu*8*32*j + delta rows: waves with j - 1, j and j + 1 tiles, a
ragged last tile, waves with no tile at all (j = 1, delta < 0). K = 300 (Kpad >
256) runs the path without the prefetch. Rows outside the f16 range or
non-finite sit in the first, a middle and the last tile."""
import numpy as np
import pytest

import oracle
from amd import lshkm
from conftest import assert_dist

pytestmark = pytest.mark.gpu

D, L, KF, W = 128, 5, 4, 0.4
SMALL_N = (1, 31, 32, 33, 255, 256, 257)
STATS = ("STAT_HASH_EXACT", "STAT_ASSIGN_AMBIG", "STAT_REFINED", "STAT_HASH_FIX", "STAT_POW_FIX")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


@pytest.fixture(scope="module")
def params():
    V, t, r, _ = lshkm.params_lsh_euclidean(4242, L, KF, D, W)
    return V, t, r


def boundary_n(ctx):
    cu = ctx.torch.cuda.get_device_properties(0).multi_processor_count
    return [cu * 8 * 32 * j + dl for j in (1, 2, 3) for dl in (-33, -1, 0, 1, 33)], cu * 8 * 32 * 3 + 33


def bad_rows(N):
    """Rows x_ok refuses, in the first, a middle and the last tile (N >= 31)."""
    if N < 31:
        return []
    mid = (((N + 31) // 32) // 2) * 32
    return sorted({1, 2, min(mid + 5, N - 1), min(mid + 6, N - 1), N - 2, N - 1})


def make_rows(ctx, N, kind, seed):
    X = ctx.synth(seed, N, D, kind=kind)
    vals = ((3, np.float32(3e38)), (70, np.float32(np.inf)), (5, np.float32(np.nan)),
            (100, np.float32(-3e38)), (40, np.float32(-np.inf)), (127, np.float32(np.nan)))
    for i, (col, v) in zip(bad_rows(N), vals):
        X[i, col] = float(v)
    return X


def centroids(ctx, K, seed):
    # centroids of the rows' own scale (not dataset rows: no exact zero distances
    # whose certified value would have to be bit-exact by luck of the draw)
    Ch = oracle.synth(seed, K, D, kind="normal").astype(np.float64) * (1.0 + 2.0 ** -30)
    if K > 9:
        Ch[9] = Ch[4]                               # a tie: the lower index wins
    return Ch


def same(got, want, what):
    """Bit for bit, compared on the device (fp64 distances as int64: NaN == NaN)."""
    import torch
    for i, (g, w) in enumerate(zip(got, want)):
        if g.dtype.is_floating_point:
            g, w = g.view(torch.int64), w.view(torch.int64)
        assert g.shape == w.shape and bool((g == w).all()), (what, i)


def check_dist(got, want, mode):
    fin = np.isfinite(want)
    assert_dist(got[fin], want[fin], mode)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])


def counters(c):
    return tuple(c.stat(getattr(lshkm, s)) for s in STATS)


def run_hash_assign(M, c, params, X, C, nb):
    V, t, r = params
    lsh = M.LSH(c, "euclidean", D, KF, L, nb, W, V=V, t=t, r=r)
    c.reset_stats()
    tu, ph, bu, a, d = M.hash_assign(lsh, X, C, tuples=True, phi=True, bucket=True)
    c.sync()
    return [tu, ph, bu, a, d], counters(c)


def run_lloyd(M, c, X, C):
    c.reset_stats()
    a, d = M.lloyd_assign(c, X, C, "euclidean")
    c.sync()
    return [a, d], counters(c)


def check_case(ctx, sctx, sw, monkeypatch, params, N, K, kind, with_oracle):
    X = make_rows(ctx, N, kind, 0x9F00 + N % 9973 + K)
    Ch = centroids(ctx, K, 77 + K)
    C = ctx.torch.from_numpy(Ch).to(ctx.dev)
    nb = max(N // 100, 1)
    V, t, r = params
    what = (N, K, kind)
    # the product: hashing + Lloyd in one pass, and Lloyd alone (HASH = false)
    ha, _ = run_hash_assign(lshkm, ctx, params, X, C, nb)
    la, _ = run_lloyd(lshkm, ctx, X, C)
    # LSH outputs against the standalone MFMA hash, bit for bit
    ref_lsh = list(lshkm.LSH(ctx, "euclidean", D, KF, L, nb, W, V=V, t=t, r=r).hash(X))
    same(ha[:3], ref_lsh, ("hash", what))
    # the exact mode (the gather-ring kernels): the same cluster IDs, distances within DIST_TOL
    ctx.set_dist_mode("exact")
    try:
        xa, _ = run_hash_assign(lshkm, ctx, params, X, C, nb)
    finally:
        ctx.set_dist_mode("certified")
    same(xa[:3], ref_lsh, ("hash, exact mode", what))
    xd = xa[4].cpu().numpy()
    for got in (ha[3:], la):
        same(got[:1], xa[3:4], ("cluster IDs", what))
        check_dist(got[1].cpu().numpy(), xd, "certified")
    if with_oracle:
        Xh = X.cpu().numpy()
        sub = np.unique(np.r_[0:min(64, N), max(N - 64, 0):N])
        ot, op, ob = oracle.lsh_hash_euclid(Xh[sub], V, t, np.float32(W), r, nb)
        for g, o in zip(ha[:3], (ot, op, ob)):
            assert np.array_equal(g.cpu().numpy()[sub], o), ("hash vs oracle", what)
        oa, od = oracle.lloyd_assign(Xh[sub], Ch, "euclidean", None)
        assert np.array_equal(ha[3].cpu().numpy()[sub], oa), ("cluster IDs vs oracle", what)
        check_dist(xd[sub], od, "exact")
        check_dist(ha[4].cpu().numpy()[sub], od, "certified")
    # the test build, prefetch on and off: identical outputs and counters
    res = {}
    for sw_env in (None, "0"):
        if sw_env is not None:
            monkeypatch.setenv("LSHKM_ROW_PREFETCH", sw_env)
        try:
            res[sw_env] = (run_hash_assign(sw, sctx, params, X, C, nb), run_lloyd(sw, sctx, X, C))
        finally:
            monkeypatch.delenv("LSHKM_ROW_PREFETCH", raising=False)
    for i in range(2):
        same(res[None][i][0], res["0"][i][0], ("switch", i, what))
        assert res[None][i][1] == res["0"][i][1], ("counters", i, what, res[None][i][1], res["0"][i][1])
    same(res[None][0][0], ha, ("test build vs product", what))
    same(res[None][1][0], la, ("test build vs product, Lloyd", what))


@pytest.mark.parametrize("kind", ["grid", "normal"])
@pytest.mark.parametrize("K", [3, 64, 200, 256, 300])
def test_small_n(ctx, sctx, sw, monkeypatch, params, K, kind):
    for N in SMALL_N:
        check_case(ctx, sctx, sw, monkeypatch, params, N, K, kind, True)


@pytest.mark.parametrize("kind", ["grid", "normal"])
@pytest.mark.parametrize("K", [3, 64, 200, 256, 300])
def test_tile_boundary_n(ctx, sctx, sw, monkeypatch, params, K, kind):
    ns, n_oracle = boundary_n(ctx)
    for N in ns:
        check_case(ctx, sctx, sw, monkeypatch, params, N, K, kind, N == n_oracle)
