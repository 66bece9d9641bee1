"""GPU parity: pam_lloyds (update.hpp:89-142) — medoid rows, the swapped flag
and the winning dist_sum bits against the reference's golden outputs
(tests/golden/pam, tools/gen_pam_golden.cpp) and against an expectation built
here from the pinned oracle's exact distances; the product library, the test
build with the exact chain forced and the test build with the MFMA screen
forced must all agree."""
import glob
import os

import numpy as np
import pytest

import oracle
from amd import lshkm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

PAM_GOLDEN = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "pam", "*.npz")))
METRICS = ["euclidean", "cosine"]
BUILDS = ["product", "exact", "screen"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def to_dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a)).to(ctx.dev)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def run(build, ctx, sw, sctx, monkeypatch, Xh, assign, K, metric, prev=None, C_old=None):
    """pam_update on one of the three builds/switches; (rows, C_new numpy, sums, swapped)."""
    if build == "product":
        mod, c = lshkm, ctx
        monkeypatch.delenv("LSHKM_PAM_PATH", raising=False)
    else:
        mod, c = sw, sctx
        monkeypatch.setenv("LSHKM_PAM_PATH", build)
    Co = None if C_old is None else to_dev(c, C_old)
    med, Cn, sums, swapped = mod.pam_update(c, to_dev(c, Xh), to_dev(c, np.asarray(assign, np.int32)), K, metric, prev, Co)
    monkeypatch.delenv("LSHKM_PAM_PATH", raising=False)
    return med, None if Cn is None else Cn.cpu().numpy(), sums, swapped


def row_variants(x64):
    """fp64 rows, and fp32 rows too when every value is an fp32 value."""
    x32 = x64.astype(np.float32)
    out = [x64]
    if np.array_equal(x32.astype(np.float64), x64):
        out.append(x32)
    return out


# ------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", PAM_GOLDEN)
def test_pam_golden(ctx, sw, sctx, monkeypatch, name, build):
    g = np.load(os.path.join(GOLDEN, "pam", name + ".npz"))
    metric = METRICS[int(g["metric"][0])]
    K = len(g["prev_rows"])
    for Xh in row_variants(g["x"]):
        prev = g["prev_rows"]
        for sfx in ("", "2"):       # the second run starts from the first one's medoids
            med, _, sums, swapped = run(build, ctx, sw, sctx, monkeypatch, Xh, g["assign"], K, metric, prev)
            assert np.array_equal(med, g["medoid_rows" + sfx]), (name, build, Xh.dtype, sfx, med, g["medoid_rows" + sfx])
            assert swapped == bool(g["swapped" + sfx][0]), (name, build, sfx)
            assert np.array_equal(bits(sums), bits(g["sums" + sfx])), (name, build, sfx, sums, g["sums" + sfx])
            prev = med


def test_pam_golden_present():
    assert len(PAM_GOLDEN) >= 8, PAM_GOLDEN


# --------------------------------------------- 2. generated, independent expectation
def expect_pam(Xh, assign, K, metric, prev):
    """pam_lloyds restated: exact distances from the pinned oracle (one centroid:
    the minimum is that distance), sequential numpy adds in member order, the
    literal selection loop. Returns (rows, sums, swapped); an empty cluster keeps
    prev and the -1 sentinel."""
    rows = np.full(K, -1, np.int32)
    sums = np.full(K, -1.0)
    swapped = False
    for c in range(K):
        mem = np.nonzero(assign == c)[0]
        if len(mem) == 0:
            rows[c] = prev[c]
            continue
        Xm = np.ascontiguousarray(Xh[mem])
        # D[j, p] = dist(x_j, x_p) = dist(x_p, x_j) (bitwise symmetric)
        D = np.stack([oracle.lloyd_assign(Xm, Xm[p:p + 1].astype(np.float64), metric)[1] for p in range(len(mem))], axis=1)
        s = np.zeros(len(mem))
        with np.errstate(invalid="ignore"):
            for j in range(len(mem)):
                s = s + D[j, :]
        mn, best = -1.0, 0
        for p in range(len(mem)):
            if mn == -1 or s[p] < mn:
                mn, best = s[p], p
        rows[c], sums[c] = mem[best], mn
        swapped |= bool(prev[c] < 0 or mem[best] != prev[c])
    return rows, sums, swapped


SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 129, 257, 0]      # cluster 11 is empty


def planted_assign(seed):
    a = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(SIZES)])
    return np.random.RandomState(seed).permutation(a)


def gen_rows(kind, d, N, dtype, zero_every=0):
    Xh = oracle.synth(700 + d, N, d, kind="normal" if kind == "normal" else "grid")
    if kind == "wide":
        Xh[::7, min(3, d - 1)] *= np.float32(2.0 ** 12)
    Xh = Xh.astype(dtype)
    if dtype == np.float64 and kind == "normal":
        Xh = Xh * (1.0 + 2.0 ** -30) + 2.0 ** -40         # general doubles: no fp32 image
    if zero_every:
        Xh[::zero_every] = 0.0
    return Xh


_EXPECT = {}


def case_expect(key, Xh, assign, K, metric, prev):
    if key not in _EXPECT:
        _EXPECT[key] = expect_pam(Xh, assign, K, metric, prev)
    return _EXPECT[key]


@pytest.mark.parametrize("d,kind,dtype,metric,zero_every", [
    (4, "grid", np.float32, "euclidean", 0),
    (8, "normal", np.float64, "euclidean", 0),
    (100, "wide", np.float32, "euclidean", 0),
    (128, "normal", np.float32, "euclidean", 0),
    (128, "grid", np.float64, "euclidean", 0),
    (600, "grid", np.float32, "euclidean", 0),            # above the exact kernel's LDS row limit (512)
    (8, "grid", np.float32, "cosine", 101),               # zero rows; row 0 is a zero first member
    (100, "normal", np.float64, "cosine", 101),
    # d % 4 != 0: the scalar tail of sil_euclid (pairsum.h) and the screen's
    # element-wise staging loop (clusters of >= 64 members take the screen)
    (1, "grid", np.float32, "euclidean", 0),
    (3, "normal", np.float32, "euclidean", 0),
    (7, "normal", np.float64, "euclidean", 0),            # general doubles
    (33, "wide", np.float32, "euclidean", 0),
    (513, "grid", np.float32, "euclidean", 0),
    (5, "grid", np.float32, "cosine", 101),
])
def test_pam_generated(ctx, sw, sctx, monkeypatch, d, kind, dtype, metric, zero_every):
    K = len(SIZES)
    assign = planted_assign(d)
    N = len(assign)
    assert N <= 3000
    Xh = gen_rows(kind, d, N, dtype, zero_every)
    if zero_every:
        assert not Xh[np.nonzero(assign == assign[0])[0][0]].any()    # a zero row leads its cluster
    prev = np.full(K, -1, np.int32)
    prev[K - 1] = 5                                        # the empty cluster's previous centroid
    C_old = Xh[np.arange(K) * 7].astype(np.float64)
    erows, esums, esw = case_expect((d, kind, str(dtype), metric), Xh, assign, K, metric, prev)
    got = {}
    for build in BUILDS:
        med, Cn, sums, swapped = run(build, ctx, sw, sctx, monkeypatch, Xh, assign, K, metric, prev, C_old)
        assert np.array_equal(med, erows), (build, med, erows)
        assert np.array_equal(bits(sums), bits(esums)), (build, sums, esums)
        assert swapped == esw, build
        want_C = Xh[np.where(med >= 0, med, 0)].astype(np.float64)
        want_C[K - 1] = C_old[K - 1]                      # the empty cluster keeps its centroid
        assert np.array_equal(bits(Cn), bits(want_C)), build
        got[build] = (med, sums, swapped)
    assert med[K - 1] == 5 and esums[K - 1] == -1.0


# ---------------------------------------------------------------------- 3. ties
def test_pam_ties(ctx, sw, sctx, monkeypatch):
    d = 16
    Xh = oracle.synth(31, 140, d).astype(np.float32)
    assign = np.repeat(np.arange(2, dtype=np.int32), 70)
    # each cluster's medoid becomes the cluster mean on the grid, present twice
    for c, (r1, r2) in enumerate([(10, 40), (135, 75)]):
        mem = np.nonzero(assign == c)[0]
        centre = np.round(Xh[mem].astype(np.float64).mean(axis=0) * 2 ** 15) / 2 ** 15
        Xh[r1] = Xh[r2] = centre.astype(np.float32)
    prev = np.array([-1, -1], np.int32)
    erows, esums, _ = expect_pam(Xh, assign, 2, "euclidean", prev)
    assert list(erows) == [10, 75]                          # the copies hold the minimum: the lower row wins
    for build in BUILDS:
        if build == "screen":
            sctx.reset_stats()
        med, _, sums, _ = run(build, ctx, sw, sctx, monkeypatch, Xh, assign, 2, "euclidean", prev)
        assert list(med) == [10, 75], (build, med)
        assert np.array_equal(bits(sums), bits(esums)), build
        if build == "screen":
            left = sctx.stat(sw.STAT_PAM_EXACT)
            assert sctx.stat(sw.STAT_PAM_SCREENED) == 2
            assert left >= 4, f"both copies of both medoids must reach the exact chain, stat 11 = {left}"


# ------------------------------------------------- 4. the screen ran and screened
def test_pam_screen_screens(sw, sctx, monkeypatch):
    d, n = 128, 257
    sizes = [n, 1, 40]
    assign = np.random.RandomState(4).permutation(np.concatenate([np.full(m, c, np.int32) for c, m in enumerate(sizes)]))
    Xh = oracle.synth(77, len(assign), d).astype(np.float32)
    mem = np.nonzero(assign == 0)[0]
    # numpy restatement on the CPU: the gap between the best and the second-best
    # sum must be far above any plausible bound (else plant the medoid at the mean)
    def gap():
        Xm = Xh[mem].astype(np.float64)
        D = np.sqrt(np.maximum(((Xm[:, None, :] - Xm[None, :, :]) ** 2).sum(-1), 0.0))
        s = np.sort(D.sum(axis=1))
        return (s[1] - s[0]) / s[0]
    if gap() < 1e-3:
        Xh[mem[5]] = (np.round(Xh[mem].astype(np.float64).mean(axis=0) * 2 ** 15) / 2 ** 15).astype(np.float32)
    assert gap() >= 1e-3, gap()
    prev = np.full(3, -1, np.int32)
    erows, esums, _ = expect_pam(Xh, assign, 3, "euclidean", prev)
    sctx.reset_stats()
    monkeypatch.setenv("LSHKM_PAM_PATH", "screen")
    med, _, sums, _ = sw.pam_update(sctx, to_dev(sctx, Xh), to_dev(sctx, assign), 3, "euclidean", prev)
    screened, left = sctx.stat(sw.STAT_PAM_SCREENED), sctx.stat(sw.STAT_PAM_EXACT)
    assert np.array_equal(med, erows) and np.array_equal(bits(sums), bits(esums))
    print(f"pam screen forced: stat 10 = {screened}, stat 11 = {left} of {len(assign)} members")
    assert screened == 2, screened                          # the clusters of >= 2 members
    assert left < len(assign), f"stat 11 = {left} of {len(assign)} members reached the exact chain"
    assert left >= 2                                        # at least each screened cluster's winner
    # exact-only: neither counter moves
    sctx.reset_stats()
    monkeypatch.setenv("LSHKM_PAM_PATH", "exact")
    sw.pam_update(sctx, to_dev(sctx, Xh), to_dev(sctx, assign), 3, "euclidean", prev)
    assert sctx.stat(sw.STAT_PAM_SCREENED) == 0 and sctx.stat(sw.STAT_PAM_EXACT) == 0


# ------------------------------------------------------ 5. prev_rows / swapped
def test_pam_prev_rows_swapped(ctx):
    K = 5
    Xh = oracle.synth(12, 400, 8).astype(np.float32)
    assign = (np.arange(400) % K).astype(np.int32)
    X, a = to_dev(ctx, Xh), to_dev(ctx, assign)
    med, Cn, _, swapped = lshkm.pam_update(ctx, X, a, K, "euclidean")            # NULL
    assert swapped and Cn is None
    med2, _, _, swapped2 = lshkm.pam_update(ctx, X, a, K, "euclidean", np.full(K, -1, np.int32))
    assert swapped2 and np.array_equal(med, med2)
    med3, _, _, swapped3 = lshkm.pam_update(ctx, X, a, K, "euclidean", med)      # the answer itself
    assert not swapped3 and np.array_equal(med, med3)
    other = med.copy()
    other[3] = [r for r in np.nonzero(assign == 3)[0] if r != med[3]][0]
    med4, _, _, swapped4 = lshkm.pam_update(ctx, X, a, K, "euclidean", other)    # one cluster differs
    assert swapped4 and np.array_equal(med, med4)


# ------------------------------------------------------------- 6. argument errors
def test_pam_argument_errors(ctx):
    Xh = oracle.synth(13, 64, 8).astype(np.float32)
    X = to_dev(ctx, Xh)
    for bad in (4, -1):
        assign = (np.arange(64) % 4).astype(np.int32)
        assign[17] = bad
        with pytest.raises(lshkm.LshkmError, match="outside"):
            lshkm.pam_update(ctx, X, to_dev(ctx, assign), 4, "euclidean")
    assign = to_dev(ctx, (np.arange(64) % 4).astype(np.int32))
    med = np.empty(4, np.int32)
    sw_ = lshkm.C.c_int()
    Cn = ctx.empty((4, 8), ctx.torch.float64)
    rc = lshkm.lib().lshkm_pam_update(ctx.h, lshkm._t_ptr(X), 64, 8, lshkm._t_ptr(assign), 4, 0, None, None,
                                      lshkm._np_ptr(med), lshkm._t_ptr(Cn), None, lshkm.C.byref(sw_))
    assert rc == -1, rc                                     # LSHKM_ERR_ARG: C_new without C_old
    # the context still works
    assert lshkm.pam_update(ctx, X, assign, 4, "euclidean")[3]


# ------------------------------------------------------------ 7. cluster.py, pam
def test_cluster_vectors_pam(ctx):
    import importlib.util
    from amd import PKG
    spec = importlib.util.spec_from_file_location("cluster_amd_pam", os.path.join(PKG, "cluster.py"))
    cluster = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cluster)
    N, K, d = 2000, 8, 16
    Xh = oracle.synth(55, N, d)
    res = cluster.cluster_vectors(ctx, Xh, K, 200, 0.0, 7, metric="euclidean", update="pam")
    assert not res["cont"] and res["iters"] < 200, res["iters"]          # a fixed point: no medoid swapped
    rows = res["medoid_rows"]
    assert np.array_equal(bits(res["centers"]), bits(Xh[rows].astype(np.float64)))
    assert np.array_equal(res["assign"][rows], np.arange(K))            # the override of lloyds_assignment
    # one more update from the fixed point changes nothing
    med, _, _, swapped = lshkm.pam_update(ctx, to_dev(ctx, Xh), to_dev(ctx, res["assign"]), K, "euclidean", rows)
    assert not swapped and np.array_equal(med, rows)
