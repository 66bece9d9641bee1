"""GPU: the FAST hash+assign kernel's tile-pair loop and its leaner hash finish.

fused_hi_kernel<.., FAST, PF, HG> (csrc/fused_hi.hip; K <= 256, euclidean,
certified mode, fp32 rows of 128 dims) runs a wave's tiles in pairs, the two
register sets of the rows' upper halves trading places, with a single last tile
through the first copy of the body; it reads a table's constants as four 16-B
LDS reads, sums the table's four phi terms in one wrapping expression
(tile.h phi_sum4_small) and, for L = 5 or 6, does not accumulate the hash
tile's registers that hold no function (HG = 3).

Row counts: with cu compute units of 8 waves of 32-row tiles, cu*8*32*j + delta
rows for j in {1, 2, 4, 5} and delta in {-33, -1, 0, 1, 33}: waves with 0..6
tiles, that is whole pairs, a pair plus a single tile, a single tile, and a
ragged last tile; and 1, 31, 32, 33, 63, 64, 65 rows. LSH shapes: k = 4 with
L in {1, 2, 5, 6, 8} (one live group; the headline's three, group 2 live in one
and in both lane halves; all four), the bucket count N // 100 and a single
bucket. K in {3, 32, 256, 300}; 300 (Kpad > 256) runs the path without the
pair loop. The LSH shapes and the K values run at a small and at a boundary
row count each, the row counts at the headline's shape: the cross product of
the three lists would be 1,080 cases of the same code.

Checks, each case: tuples, phi, bucket and cluster IDs bit for bit against the
CPU oracle (on the rows of the first and last tiles, of the tiles around every
multiple of cu*8*32 rows, where the waves' tile counts change, and on every
211th row), distances through conftest.assert_dist; outputs and the five
counters identical to the same call under LSHKM_ROW_PREFETCH=0 in the test
build (every row), and to the product build; and identical when the same
context runs the call a second time.

Large hash values, and where the summed phi's result reaches the output. The
fix-up (hash_fixup_kernel) recomputes phi and bucket of every table that has an
uncertified function, with tile.h's phi_term: phi_sum4_small's value survives
only in tables whose four functions pass the f32 certificate
(hash_tile.h certify_floor_f32), floor(y - B) == floor(y + B) with
  B = |y| G + nxf P_f + Q_f,  G = 1.19e-6,  P_f = (A1H |v| + A2 sqrt(d)) / w
(hash_window; A1H = 1.25 2^-18, |v| ~ 11.3, w = 0.4: P_f ~ 1.36e-4 per unit of
|x|, the same for every function of the row whatever its direction). For a row
aligned with a projection vector, |y| ~ 28.3 |x|, so B ~ 1.70e-4 |x|: B reaches
0.5 at |x| ~ 2,900, |h| ~ 2^16.3, and no table of a longer row is certified.
Three legs:
- test_certified_large_hash_values: rows aligned with one function, both signs,
  |h| of that function in [2^15, 2^15.1], each row moved by a tiny delta (the
  minimum-norm solution of 4 L linear equations) so that every one of its 4 L
  values y lies at an integer + 1/2. The test restates B on the CPU (fp64, its
  terms rounded up by 1e-3) and requires dist(y, Z) > 2 B for every function
  of every row: the kernel's y~ lies within B of y (the certificate's own
  bound), so y~ -+ B cannot cross an integer and the kernel must certify every
  function. It asserts that the call lists no row for the hash fix-up (counter
  STAT_HASH_FIX == 0), so every phi and bucket of the output is the summed
  form's, and compares tuples, phi and buckets of every row with the oracle.
  r of the aligned functions is 0 and 100 in turn (and the generator's values).
- the same construction up to |h| ~ 2^16.3 (B up to ~0.48): certified by the
  kernel wherever its actual error leaves room, which the test cannot know
  beforehand; every row against the oracle, no floor asserted.
- test_fixup_path_large_hash_values: f16-range rows (|x| up to 2^14.9) aligned
  with one function, |h| up to 2^19.8 with both signs. None of their tables can
  be certified: this is the fix-up path, on which the summed phi runs on values
  outside its contract first (any int32 h gives it the same bits as the
  term-by-term form: tests/test_phi_sum_cpu.py) and is then overwritten. The
  rows that make_rows scales by 2^9..2^11 (|x| >= 5,800) are of this kind too."""
import numpy as np
import pytest

import oracle
from amd import lshkm
from conftest import assert_dist

pytestmark = pytest.mark.gpu

D, KF, W = 128, 4, 0.4
SMALL_N = (1, 31, 32, 33, 63, 64, 65)
DELTAS = (-33, -1, 0, 1, 33)
STATS = ("STAT_HASH_EXACT", "STAT_ASSIGN_AMBIG", "STAT_REFINED", "STAT_HASH_FIX", "STAT_POW_FIX")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


@pytest.fixture(scope="module")
def unit(ctx):
    """Rows of one tile per wave: cu * 8 * 32."""
    return ctx.torch.cuda.get_device_properties(0).multi_processor_count * 8 * 32


_PARAMS = {}


def lsh_params(L):
    if L not in _PARAMS:
        V, t, r, _ = lshkm.params_lsh_euclidean(4242 + L, L, KF, D, W)
        _PARAMS[L] = (V, t, r)
    return _PARAMS[L]


_CENTROIDS = {}


def centroids(K):
    # the rows' own scale, not dataset rows: no exact zero distances
    if K not in _CENTROIDS:
        Ch = oracle.synth(77 + K, K, D, kind="normal").astype(np.float64) * (1.0 + 2.0 ** -30)
        if K > 9:
            Ch[9] = Ch[4]                               # a tie: the lower index wins
        _CENTROIDS[K] = Ch
    return _CENTROIDS[K]


def make_rows(ctx, N, seed):
    """N(0,1)-like rows (|h| up to ~100, nearly all certified); every 7th row
    scaled by +-2^9 .. +-2^11 (|x| >= 5,800: hash values of thousands to 2^16 of
    both signs, every function uncertified, so these rows take the fix-up path)."""
    X = ctx.synth(seed, N, D, kind="normal")
    idx = np.arange(3, N, 7)
    if idx.size:
        sc = (2.0 ** (9 + idx % 3)) * np.where(idx % 2 == 0, 1.0, -1.0)
        ti = ctx.torch.from_numpy(idx).to(ctx.dev)
        X[ti] = X[ti] * ctx.torch.from_numpy(sc.astype(np.float32)).to(ctx.dev)[:, None]
    return X


def oracle_rows(N, unit):
    """First and last tiles, the tiles around every multiple of `unit` rows, every 211th row."""
    parts = [np.arange(0, min(96, N)), np.arange(max(N - 96, 0), N), np.arange(0, N, 211)]
    for m in range(unit, N + 64, unit):
        parts.append(np.arange(max(m - 64, 0), min(m + 64, N)))
    return np.unique(np.concatenate(parts))


def same(got, want, what):
    """Bit for bit, compared on the device (fp64 distances as int64: NaN == NaN)."""
    import torch
    for i, (g, w) in enumerate(zip(got, want)):
        if g.dtype.is_floating_point:
            g, w = g.view(torch.int64), w.view(torch.int64)
        assert g.shape == w.shape and bool((g == w).all()), (what, i)


def counters(c):
    return tuple(c.stat(getattr(lshkm, s)) for s in STATS)


def run_hash_assign(M, c, params, L, X, C, nb):
    V, t, r = params
    lsh = M.LSH(c, "euclidean", D, KF, L, nb, W, V=V, t=t, r=r)
    out = []
    for _ in range(2):                                  # the same context, the same call twice
        c.reset_stats()
        tu, ph, bu, a, d = M.hash_assign(lsh, X, C, tuples=True, phi=True, bucket=True)
        c.sync()
        out.append(([tu.clone(), ph.clone(), bu.clone(), a.clone(), d.clone()], counters(c)))
    return out


def check_case(ctx, sctx, sw, monkeypatch, unit, N, K, L, nb, X=None, params=None, hash_all=False):
    """hash_all: the LSH outputs of every row against the oracle (Lloyd on the
    subset as ever). Returns the oracle's tuples of the rows compared and the
    product call's counters."""
    what = (N, K, L, nb)
    params = params or lsh_params(L)
    V, t, r = params
    if X is None:
        X = make_rows(ctx, N, 0x51A0 + N % 9973 + K + L)
    Ch = centroids(K)
    C = ctx.torch.from_numpy(Ch).to(ctx.dev)
    first, second = run_hash_assign(lshkm, ctx, params, L, X, C, nb)
    same(second[0], first[0], ("second call", what))
    assert second[1] == first[1], ("counters, second call", what, first[1], second[1])
    ha = first[0]
    # the CPU oracle
    sub = oracle_rows(N, unit)
    Xs = X[ctx.torch.from_numpy(sub).to(ctx.dev)].cpu().numpy()
    si = ctx.torch.from_numpy(sub).to(ctx.dev)
    if hash_all:
        ot, op, ob = oracle.lsh_hash_euclid(X.cpu().numpy(), V, t, np.float32(W), r, nb)
        for name, g, o in zip(("tuples", "phi", "bucket"), ha[:3], (ot, op, ob)):
            assert np.array_equal(g.cpu().numpy(), o), (name + " vs oracle, every row", what)
    else:
        ot, op, ob = oracle.lsh_hash_euclid(Xs, V, t, np.float32(W), r, nb)
        for name, g, o in zip(("tuples", "phi", "bucket"), ha[:3], (ot, op, ob)):
            assert np.array_equal(g[si].cpu().numpy(), o), (name + " vs oracle", what)
    oa, od = oracle.lloyd_assign(Xs, Ch, "euclidean", None)
    assert np.array_equal(ha[3][si].cpu().numpy(), oa), ("cluster IDs vs oracle", what)
    assert_dist(ha[4][si].cpu().numpy(), od, "certified")
    # the test build with the pair loop and with the plain loop (rows loaded at the tile's top)
    res = {}
    for sw_env in (None, "0"):
        if sw_env is not None:
            monkeypatch.setenv("LSHKM_ROW_PREFETCH", sw_env)
        try:
            res[sw_env] = run_hash_assign(sw, sctx, params, L, X, C, nb)
        finally:
            monkeypatch.delenv("LSHKM_ROW_PREFETCH", raising=False)
    for i in range(2):
        same(res[None][i][0], res["0"][i][0], ("switch", i, what))
        assert res[None][i][1] == res["0"][i][1], ("counters", i, what, res[None][i][1], res["0"][i][1])
    same(res[None][0][0], ha, ("test build vs product", what))
    assert res[None][0][1] == first[1], ("counters, test build vs product", what)
    return ot, first[1]


def rule_nb(N):
    return max(N // 100, 1)


def test_small_row_counts(ctx, sctx, sw, monkeypatch, unit):
    for N in SMALL_N:
        check_case(ctx, sctx, sw, monkeypatch, unit, N, 256, 5, rule_nb(N))


@pytest.mark.parametrize("j", [1, 2, 4, 5])
def test_pair_row_counts(ctx, sctx, sw, monkeypatch, unit, j):
    for dl in DELTAS:
        N = unit * j + dl
        check_case(ctx, sctx, sw, monkeypatch, unit, N, 256, 5, rule_nb(N))


@pytest.mark.parametrize("single_bucket", [False, True])
@pytest.mark.parametrize("L", [1, 2, 5, 6, 8])
def test_lsh_shapes(ctx, sctx, sw, monkeypatch, unit, L, single_bucket):
    for N in (65, unit * 2 + 33, unit * 3 - 1):
        check_case(ctx, sctx, sw, monkeypatch, unit, N, 32, L, 1 if single_bucket else rule_nb(N))


@pytest.mark.parametrize("K", [3, 32, 256, 300])
def test_k(ctx, sctx, sw, monkeypatch, unit, K):
    for N in (33, unit + 1, unit * 3 + 33):
        check_case(ctx, sctx, sw, monkeypatch, unit, N, K, 5, rule_nb(N))


def aligned_params(L):
    """The generator's parameters with r of functions 0 and 1 of every table set to 0 and 100."""
    V, t, r = lsh_params(L)
    r = r.copy()
    rf = r.reshape(-1)
    rf[0::4] = 0
    rf[1::4] = 100
    return V, t, r


def window_bound(Xh, V, t):
    """y (fp64, from the fp32 rows) and an upper bound of certify_floor_f32's B
    for every row and function: hash_window's P_f and Q_f restated in fp64 from
    |v|_2 and |v|_1, every term rounded up by 1e-3 (the kernel's f32 roundings,
    its nxf and pnorm inflations are below 2^-15 relative), |y~| <= |y| + 1."""
    A1H, A2, G = 1.25 * 2.0 ** -18, 2.0 ** -24, (2.0 ** -22 + 2.0 ** -20) * (1.0 + 2.0 ** -18)
    w = float(np.float32(W))
    Vf = V.reshape(-1, D).astype(np.float64)
    tf = t.reshape(-1).astype(np.float64)
    x = Xh.astype(np.float64)
    y = (x @ Vf.T + tf) / w
    P = (A1H * np.linalg.norm(Vf, axis=1) + A2 * np.sqrt(D)) / w
    Q = (A2 * np.abs(Vf).sum(axis=1) + (2.0 ** -40 + 2.0 ** -23) * np.abs(tf)) / w + 2.0 ** -126
    nx = np.linalg.norm(x, axis=1)
    B = ((np.abs(y) + 1.0) * G + nx[:, None] * P[None, :] + Q[None, :]) * 1.001
    return y, B


def aligned_rows(V, t, N, h_lo, h_hi):
    """Row i aligned with function i % (4 L), sign alternating every 3 rows, that
    function's |h| spread over [h_lo, h_hi]; then the minimum-norm delta that puts
    every one of the row's 4 L values y at an integer + 1/2."""
    w = float(np.float32(W))
    Vf = V.reshape(-1, D).astype(np.float64)
    tf = t.reshape(-1).astype(np.float64)
    LK = Vf.shape[0]
    rows = np.arange(N)
    f = rows % LK
    hmag = h_lo * (h_hi / h_lo) ** (((rows // LK) % 16) / 15.0)
    sign = np.where((rows // 3) % 2 == 0, 1.0, -1.0)
    vn = np.linalg.norm(Vf[f], axis=1)
    x = Vf[f] / vn[:, None] * (hmag * w / vn * sign)[:, None]
    x += oracle.synth(0xA11, N, D, kind="normal").astype(np.float64) * 0.25
    pinv = np.linalg.pinv(Vf)                                   # [D, LK]
    for _ in range(2):                                          # the second round takes up the fp32 rounding of the first
        y = (x.astype(np.float32).astype(np.float64) @ Vf.T + tf) / w
        x = x + (w * (np.floor(y) + 0.5 - y)) @ pinv.T
    return x.astype(np.float32), f


@pytest.mark.parametrize("L", [1, 5, 8])
def test_certified_large_hash_values(ctx, sctx, sw, monkeypatch, unit, L):
    """|h| in [2^15, 2^15.1] on rows the kernel must certify in every function:
    no row on the fix-up list, so the output's phi is phi_sum4_small's."""
    N = unit + 33
    V, t, r = aligned_params(L)
    Xh, f = aligned_rows(V, t, N, 2.0 ** 15.02, 2.0 ** 15.1)
    y, B = window_bound(Xh, V, t)
    dist = np.abs(y - np.round(y))
    # |y~ - y| <= B is the certificate's own bound: with dist(y, Z) > 2 B neither y~ - B nor y~ + B crosses an integer
    assert (dist > 2.0 * B).all(), (float((dist - 2.0 * B).min()), float(B.max()))
    X = ctx.torch.from_numpy(Xh).to(ctx.dev)
    ot, cnt = check_case(ctx, sctx, sw, monkeypatch, unit, N, 32, L, rule_nb(N), X=X, params=(V, t, r), hash_all=True)
    assert cnt[STATS.index("STAT_HASH_FIX")] == 0 and cnt[STATS.index("STAT_HASH_EXACT")] == 0, cnt
    # every row holds a certified table with |h| >= 2^15, of either sign, on functions with r = 0, 100 and the generator's
    big = np.abs(ot.reshape(N, -1)[np.arange(N), f])
    assert big.min() >= 2 ** 15 and ot.max() >= 2 ** 15 and ot.min() <= -(2 ** 15), (int(big.min()), int(ot.min()), int(ot.max()))
    assert set(np.unique(f % 4)) == {0, 1, 2, 3}


@pytest.mark.parametrize("L", [5, 8])
def test_large_hash_values_to_the_window(ctx, sctx, sw, monkeypatch, unit, L):
    """The same rows up to |h| ~ 2^16.3, where B nears 1/2: certified wherever the
    kernel's actual error leaves room. Every row against the oracle; no floor."""
    N = unit + 33
    V, t, r = aligned_params(L)
    Xh, f = aligned_rows(V, t, N, 2.0 ** 15.1, 2.0 ** 16.3)
    X = ctx.torch.from_numpy(Xh).to(ctx.dev)
    ot, _ = check_case(ctx, sctx, sw, monkeypatch, unit, N, 32, L, rule_nb(N), X=X, params=(V, t, r), hash_all=True)
    assert ot.max() >= 2 ** 16 and ot.min() <= -(2 ** 16), (int(ot.min()), int(ot.max()))


@pytest.mark.parametrize("L", [5, 8])
def test_fixup_path_large_hash_values(ctx, sctx, sw, monkeypatch, unit, L):
    """Rows aligned with projection vectors, norms from 2^11 to just under 2^15
    (the f16 range), both signs: |h| to 2^19.8, every table through the fix-up."""
    N = unit + 33
    V, t, r = aligned_params(L)
    Vf = V.reshape(L * KF, D).astype(np.float64)
    rows = np.arange(N)
    f = rows % (L * KF)
    norm = 2.0 ** (11 + (rows // (L * KF)) % 5 * 0.98)          # 2^11 .. 2^14.92
    sign = np.where((rows // 3) % 2 == 0, 1.0, -1.0)
    Xh = (Vf[f] / np.linalg.norm(Vf[f], axis=1, keepdims=True) * (norm * sign)[:, None]).astype(np.float32)
    # a little of every other direction, so the other functions are not degenerate
    Xh += oracle.synth(0xA11, N, D, kind="normal") * np.float32(0.25)
    assert np.sqrt((Xh.astype(np.float64) ** 2).sum(axis=1)).max() < 2.0 ** 15
    X = ctx.torch.from_numpy(Xh).to(ctx.dev)
    ot, _ = check_case(ctx, sctx, sw, monkeypatch, unit, N, 32, L, rule_nb(N), X=X, params=(V, t, r))
    assert ot.max() >= 2 ** 19 and ot.min() <= -(2 ** 19), (int(ot.min()), int(ot.max()))
