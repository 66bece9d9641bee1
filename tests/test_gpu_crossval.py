"""GPU parity: the LSH recommender's 10-fold validation (main.cpp:393-437,
lsh_rec_10_fold_validation_A) against fixtures written by the reference's own
functions (tests/golden/cv/*.npz, tools/gen_cv_golden.cpp) and, at a larger
size, against an expectation composed in this file from the CPU oracle plus a
numpy restatement of split_to_10 / hide_one_score / the fold loop. Every
comparison is bit for bit and covers every user."""
import ctypes
import glob
import os

import numpy as np
import pytest

import oracle
from amd import lshkm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CV = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "cv", "*.npz")))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a)).to(ctx.dev)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "cv", name + ".npz"))


def users_on_device(ctx, x, xm, up, ui):
    return dev(ctx, x), dev(ctx, xm), dev(ctx, up), dev(ctx, ui if len(ui) else np.zeros(1, np.int32))[:len(ui)]


def test_fixtures_present():
    assert CV == ["cos", "cos_bigp", "eu", "nan", "sparse"]


@pytest.mark.parametrize("name", CV)
def test_hide_matches_reference(ctx, name):
    g = load(name)
    split = g["split"]
    M = len(split)
    X, xm, up, ui = users_on_device(ctx, g["x"], g["x_mean"], g["unk_ptr"], g["unk_idx"])
    draw = np.repeat(lshkm.cv_draws([int(g["hide_seed"][0])], 1)[0], len(g["x"])).astype(np.int32)
    H, hm, hi, old = lshkm.cv_hide(ctx, X, xm, up, ui, dev(ctx, draw))
    ctx.sync()
    H, hm, hi, old = (t.cpu().numpy()[split] for t in (H, hm, hi, old))
    assert np.array_equal(hi, g["hide_idx"])
    assert np.array_equal(hi >= 0, g["hide_ret"] != 0)
    assert np.array_equal(bits(H), bits(g["h"]))
    assert np.array_equal(bits(hm), bits(g["h_mean"]))
    assert np.array_equal(bits(old), bits(g["old_score"]))
    assert M == 10 * (len(g["x"]) // 10)


@pytest.mark.parametrize("name", CV)
def test_validate10_matches_reference(ctx, name):
    g = load(name)
    metric, k, L, div, P, N, d = (int(v) for v in g["params"])
    X, xm, up, ui = users_on_device(ctx, g["x"], g["x_mean"], g["unk_ptr"], g["unk_idx"])
    mae, fs, fc, err = lshkm.lsh_validate10(ctx, X, xm, up, ui, metric, k, L, div, float(g["w"][0]), P,
                                            int(g["split_seed"][0]), int(g["hide_seed"][0]), g["lsh_seeds"], errors=True)
    err = err.cpu().numpy()
    print(name, "mae", mae, "reference", float(g["mae"][0]), "fold counts", fc.tolist())
    skipped = g["err"] == -1.0
    assert np.array_equal(err == -1.0, skipped), np.nonzero((err == -1.0) != skipped)[0][:10]
    assert np.array_equal(bits(err), bits(g["err"])), np.nonzero(bits(err) != bits(g["err"]))[0][:10]
    assert np.array_equal(fc, g["fold_cnt"].astype(np.int64))
    assert np.array_equal(bits(fs), bits(g["fold_sum"]))
    assert bits(np.array([mae]))[0] == bits(g["mae"])[0]
    # the same with one seed per user (the reference re-seeds on every call)
    mae2, fs2, fc2 = lshkm.lsh_validate10(ctx, X, xm, up, ui, metric, k, L, div, float(g["w"][0]), P,
                                          int(g["split_seed"][0]), 12345, g["lsh_seeds"],
                                          hide_seeds=np.full(N, int(g["hide_seed"][0]), np.uint64))
    assert bits(np.array([mae2]))[0] == bits(g["mae"])[0] and np.array_equal(bits(fs2), bits(fs))
    # and through the reference-named wrapper
    mae3 = lshkm.lsh_rec_10_fold_validation_A(ctx, X, xm, up, ui, "euclidean" if metric == 0 else "cosine", k, L, div,
                                              float(g["w"][0]), P, int(g["split_seed"][0]), int(g["hide_seed"][0]),
                                              g["lsh_seeds"])
    assert bits(np.array([mae3]))[0] == bits(g["mae"])[0]


@pytest.mark.parametrize("name", CV)
def test_fold_exclusion_matches_numpy_filter(ctx, name):
    """The pool of fold i as the driver sees it: a query over all rows with the
    held-out slice dropped, against a numpy filter of the same query; the sizes
    equal the reference's filtered unions (the fixture's nb_cnt)."""
    g = load(name)
    metric, k, L, div, P, N, d = (int(v) for v in g["params"])
    F = N // 10
    M = 10 * F
    split = g["split"]
    W = g["x"][split].copy()
    for i in (0, 4, 9):
        W[:(i + 1) * F] = g["h"][:(i + 1) * F]           # folds <= i in their hidden form
        Wd = dev(ctx, W)
        if metric == 0:                                   # nb = pool size / lsh_bucket_div (lsh_cube.hpp:60)
            V, t, r, _ = lshkm.params_lsh_euclidean(int(g["lsh_seeds"][i]), L, k, d, float(g["w"][0]))
            lsh = lshkm.LSH(ctx, lshkm.EUCLIDEAN, d, k, L, (M - F) // div, float(g["w"][0]), V=V, t=t, r=r)
        else:
            R, _ = lshkm.params_lsh_cosine(int(g["lsh_seeds"][i]), L, k, d)
            lsh = lshkm.LSH(ctx, lshkm.COSINE, d, k, L, R=R)
        lsh.build(Wd)
        ptr, idx = lsh.query(Wd[i * F:(i + 1) * F], True, device=True)
        eptr, eidx = lshkm.cv_exclude(ctx, ptr, idx, i * F, (i + 1) * F)
        ptr, idx, eptr, eidx = (t.cpu().numpy() for t in (ptr, idx, eptr, eidx))
        want = [idx[ptr[q]:ptr[q + 1]] for q in range(F)]
        assert sum(((s >= i * F) & (s < (i + 1) * F)).sum() for s in want) >= F     # every query finds itself
        want = [s[(s < i * F) | (s >= (i + 1) * F)] for s in want]
        assert np.array_equal(eptr, np.cumsum([0] + [len(s) for s in want]))
        assert np.array_equal(eidx, np.concatenate(want))
        nb = g["nb_cnt"][i * F:(i + 1) * F]
        asked = nb >= 0
        assert np.array_equal(np.diff(eptr)[asked], nb[asked])
        lsh.close()


def predicted_restated(X, xm, um, up, ui, nb_idx, nb_sim, nb_cnt):
    """crypto_rec.hpp:280-306 in Python floats (IEEE doubles), NaN for 0 / 0."""
    out = np.empty(len(ui), np.float64)
    for q in range(len(um)):
        for e in range(int(up[q]), int(up[q + 1])):
            index = int(ui[e])
            main_sum, abs_sum = 0.0, 0.0
            for i in range(int(nb_cnt[q])):
                cs = float(nb_sim[q, i])
                abs_sum = abs_sum + abs(cs)
                r = int(nb_idx[q, i])
                main_sum = main_sum + (cs * (float(X[r, index]) - float(xm[r])))
            with np.errstate(all="ignore"):
                out[e] = np.float64(main_sum) / np.float64(abs_sum) + np.float64(um[q])
    return out


@pytest.mark.parametrize("N,d,nq,P,levels,seed", [
    (20_000, 32, 1500, 20, 41, 1),
    (5_000, 8, 800, 15, 3, 2),            # values in {-1, 0, 1}: zero similarities, 0 / 0 scores
    (3_000, 64, 300, 64, 81, 3),
])
def test_predicted_scores_match_restatement(ctx, N, d, nq, P, levels, seed):
    rng = np.random.default_rng(seed)
    half = levels // 2
    X = rng.integers(-half, half + 1, size=(N, d)).astype(np.float64) / (8.0 if levels > 3 else 1.0)
    X[7] = 0.0
    U = rng.integers(-half, half + 1, size=(nq, d)).astype(np.float64) / (8.0 if levels > 3 else 1.0)
    xm = rng.integers(-16, 17, size=N) / 16.0
    um = rng.integers(-16, 17, size=nq) / 16.0
    sizes = rng.integers(0, 3 * P, size=nq)
    sizes[::7] = rng.integers(0, N // 2, size=len(sizes[::7]))
    cand = [np.sort(rng.choice(N, size=int(s), replace=False)).astype(np.int32) for s in sizes]
    if levels == 3:                       # users whose every similarity is 0: orthogonal candidates
        U[5] = 0.0; U[5, 0] = 1.0
        X[100:110] = 0.0; X[100:110, 1] = 1.0
        cand[5] = np.arange(100, 110, dtype=np.int32)
    cp = np.cumsum([0] + [len(c) for c in cand]).astype(np.int64)
    ci = np.concatenate(cand).astype(np.int32)
    unk = [np.sort(rng.choice(d, size=int(rng.integers(0, d + 1)), replace=False)).astype(np.int32) for _ in range(nq)]
    if levels == 3:
        unk[5] = np.array([2, 3], np.int32)
    up = np.cumsum([0] + [len(u) for u in unk]).astype(np.int64)
    ui = np.concatenate(unk).astype(np.int32)
    w_idx, w_sim, w_cnt = oracle.p_closest(X, U, cp, ci, P)
    want = predicted_restated(X, xm, um, up, ui, w_idx, w_sim, w_cnt)
    Xd, xmd = dev(ctx, X), dev(ctx, xm)
    idx, sim, cnt = lshkm.p_closest(ctx, Xd, dev(ctx, U), dev(ctx, cp), dev(ctx, ci), P)
    got = lshkm.predicted_scores(ctx, Xd, xmd, dev(ctx, um), dev(ctx, up), dev(ctx, ui), idx, sim, cnt)
    ctx.sync()
    got = got.cpu().numpy()
    if levels == 3:
        assert np.isnan(want[up[5]:up[6]]).all()
    assert np.isnan(want).any()           # users without neighbours: 0 / 0
    assert np.array_equal(bits(got), bits(want)), np.nonzero(bits(got) != bits(want))[0][:10]


def libc_draws(seed, n):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand.argtypes = [ctypes.c_uint]
    libc.rand.restype = ctypes.c_int
    libc.srand(seed)
    return [libc.rand() for _ in range(n)]


def compose_expected(x, xm, up, ui, metric, k, L, div, w, P, split_seed, hide_seed, lsh_seeds):
    """Steps 1-3 of the reference in numpy over the CPU oracle's hashing, query
    and get_P_closest: (errors in split order, fold sums, fold counts, mae)."""
    N, d = x.shape
    F = N // 10
    M = 10 * F
    draws = libc_draws(split_seed, M)
    remaining = list(range(N))
    split = np.array([remaining.pop(draws[m] % len(remaining)) for m in range(M)])
    draw = libc_draws(hide_seed, 1)[0]
    W, Wm = x[split].copy(), xm[split].copy()
    hide = np.full(M, -1)
    old = np.zeros(M)
    H, Hm = W.copy(), Wm.copy()
    for m in range(M):                                    # hide_one_score
        u = ui[up[split[m]]:up[split[m] + 1]]
        known = d - len(u)
        if known < 2:
            continue
        h = draw % known
        old[m] = H[m, h]
        H[m, u] = 0.0
        s, useless = 0.0, True
        for j in range(d):
            if j != h:
                s = s + float(H[m, j])
                useless = useless and H[m, j] == 0
        if useless:
            continue
        H[m, h] = s / (d - 1)
        Hm[m] = H[m, h]
        hide[m] = h
    err = np.full(M, -1.0)
    fs, fc = np.zeros(10), np.zeros(10, np.int64)
    all_sum = 0.0
    for i in range(10):
        sl = slice(i * F, (i + 1) * F)
        pool = np.concatenate([np.arange(0, i * F), np.arange((i + 1) * F, M)])
        Xp, xmp = W[pool], Wm[pool]                       # merge_except_for, before fold i is hidden
        W[sl], Wm[sl] = H[sl], Hm[sl]
        if metric == 0:
            nb = len(pool) // div
            V, t, r, _ = oracle.gen_lsh_euclid(int(lsh_seeds[i]), L, k, d, np.float32(w))
            tup, _, bk = oracle.lsh_hash_euclid(Xp, V, t, np.float32(w), r, nb)
            qt, _, qb = oracle.lsh_hash_euclid(W[sl], V, t, np.float32(w), r, nb)
        else:
            nb = 1 << k
            R, _ = oracle.gen_lsh_cosine(int(lsh_seeds[i]), L, k, d)
            bk, qb, tup, qt = oracle.lsh_hash_cosine(Xp, R), oracle.lsh_hash_cosine(W[sl], R), None, None
        rp, idx = oracle.bucket_csr(bk, nb)
        cand = [oracle.lsh_query(len(pool), nb, rp, idx, qb[q], tup, None if qt is None else qt[q]) for q in range(F)]
        cp = np.cumsum([0] + [len(c) for c in cand]).astype(np.int64)
        ci = np.concatenate(cand).astype(np.int32) if cp[-1] else np.zeros(0, np.int32)
        n_idx, n_sim, n_cnt = oracle.p_closest(Xp, W[sl], cp, ci, P)
        k_sum, calc = 0.0, 0
        for q in range(F):
            m = i * F + q
            if hide[m] < 0 or len(cand[q]) == 0:
                continue
            pred = predicted_restated(Xp, xmp, [Wm[m]], [0, 1], [hide[m]], n_idx[q:q + 1], n_sim[q:q + 1], n_cnt[q:q + 1])[0]
            err[m] = abs(old[m] - pred)
            k_sum = k_sum + err[m]
            calc += 1
        fs[i], fc[i] = k_sum, calc
        if calc > 0:
            all_sum = all_sum + k_sum / calc
    return err, fs, fc, all_sum / 10


@pytest.fixture(scope="module")
def composed_users():
    N, d = 1003, 17
    rng = np.random.default_rng(99)
    score = rng.integers(-64, 192, size=(N, d)) / 64.0 + rng.random((N, d)) * 2.0 ** -20
    known = rng.random((N, d)) < 0.6
    known[:, 0] |= known.sum(axis=1) == 0
    known[5] = False; known[5, 3] = True                 # one known index: not calculated
    xm = np.array([np.cumsum(np.where(known[i], score[i], 0.0))[-1] / known[i].sum() for i in range(N)])
    x = np.where(known, score, xm[:, None])
    unk = [np.nonzero(~known[i])[0].astype(np.int32) for i in range(N)]
    up = np.cumsum([0] + [len(u) for u in unk]).astype(np.int64)
    ui = np.concatenate(unk).astype(np.int32)
    return x, xm, up, ui


@pytest.mark.parametrize("metric,k,L,div,w", [(1, 4, 3, 4, 0.0), (0, 2, 3, 8, 1.0)])
def test_validate10_matches_composed_expectation(ctx, composed_users, metric, k, L, div, w):
    x, xm, up, ui = composed_users
    P = 7
    seeds = np.arange(10, dtype=np.uint64) * 77 + 5
    want_err, want_fs, want_fc, want_mae = compose_expected(x, xm, up, ui, metric, k, L, div, w, P, 2024, 31337, seeds)
    X, xmd, upd, uid = users_on_device(ctx, x, xm, up, ui)
    mae, fs, fc, err = lshkm.lsh_validate10(ctx, X, xmd, upd, uid, metric, k, L, div, w, P, 2024, 31337, seeds, errors=True)
    err = err.cpu().numpy()
    print("metric", metric, "mae", mae, "expected", want_mae, "counts", fc.tolist())
    assert want_fc.sum() > 500 and (metric == 1 or (want_err == -1.0).sum() > 1)
    assert np.array_equal(bits(err), bits(want_err)), np.nonzero(bits(err) != bits(want_err))[0][:10]
    assert np.array_equal(fc, want_fc)
    assert np.array_equal(bits(fs), bits(want_fs))
    assert bits(np.array([mae]))[0] == bits(np.array([want_mae]))[0]


def test_fewer_than_ten_users(ctx):
    x = np.arange(9 * 4, dtype=np.float64).reshape(9, 4)
    X, xm, up, ui = users_on_device(ctx, x, x.mean(axis=1), np.zeros(10, np.int64), np.zeros(0, np.int32))
    mae, fs, fc = lshkm.lsh_validate10(ctx, X, xm, up, ui, "cosine", 2, 2, 4, 0.0, 3, 1, 2, np.arange(10))
    assert mae == 0.0 and not fs.any() and not fc.any()


@pytest.mark.parametrize("metric,div,P,what", [("cosine", 4, 0, "P < 1"), ("euclidean", 1000, 3, "nb = 0"),
                                              ("euclidean", 0, 3, "lsh_bucket_div < 1")])
def test_argument_errors(ctx, metric, div, P, what):
    x = np.arange(40 * 4, dtype=np.float64).reshape(40, 4)
    X, xm, up, ui = users_on_device(ctx, x, x.mean(axis=1), np.zeros(41, np.int64), np.zeros(0, np.int32))
    with pytest.raises(lshkm.LshkmError, match="lshkm error -1"):
        lshkm.lsh_validate10(ctx, X, xm, up, ui, metric, 2, 2, div, 1.0, P, 1, 2, np.arange(10))


def test_argument_error_d(ctx):
    mae = ctypes.c_double()
    rc = lshkm.lib().lshkm_lsh_validate10(ctx.h, None, None, 40, 0, None, None, 1, 2, 2, 4, 1.0, 3, 1, 2, None, None,
                                          ctypes.byref(mae), None, None, None)
    assert rc == -1


@pytest.mark.parametrize("name", ["cos", "eu", "nan"])
def test_validate10_in_chunks_of_users(sctx, sw, monkeypatch, name):
    """The driver bounds its candidate lists by taking a fold's users in chunks
    and carrying k_sum from chunk to chunk; the test build's LSHKM_CV_CHUNK=small
    makes every fold take several chunks (64 candidate rows each, one user at
    least). Same bits as the reference."""
    monkeypatch.setenv("LSHKM_CV_CHUNK", "small")
    g = load(name)
    metric, k, L, div, P, N, d = (int(v) for v in g["params"])
    X, xm, up, ui = users_on_device(sctx, g["x"], g["x_mean"], g["unk_ptr"], g["unk_idx"])
    mae, fs, fc, err = sw.lsh_validate10(sctx, X, xm, up, ui, metric, k, L, div, float(g["w"][0]), P,
                                         int(g["split_seed"][0]), int(g["hide_seed"][0]), g["lsh_seeds"], errors=True)
    assert np.array_equal(bits(err.cpu().numpy()), bits(g["err"]))
    assert np.array_equal(fc, g["fold_cnt"].astype(np.int64))
    assert np.array_equal(bits(fs), bits(g["fold_sum"]))
    assert bits(np.array([mae]))[0] == bits(g["mae"])[0]
