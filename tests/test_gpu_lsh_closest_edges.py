"""GPU parity: lshkm_lsh_p_closest at its routing, capacity and chunk boundaries
(csrc/lshpc_layout.h is the rule, csrc/lsh_closest.hip the screen,
csrc/api_recom.cpp the chunked host loop).

tests/test_gpu_lsh_closest.py keeps every screen case at P <= 20, L * k <= 20
bits, one chunk of users and values of magnitude 1. The groups here run what
that leaves out:
  a  the kept-list capacity ladder (P 95 / 96, 223 / 224, 300, 447 / 448): the
     upper four slots per lane of the pruning wave, and the route change
  b  bucket codes of 32 bits (and 33: the lists path)
  c  row dimensions around the 32- and 128-dim instantiations
  d  user chunks (the test build's LSHKM_LSHPC_BUDGET=small: chunks of 128 users)
  e  row magnitudes 2^-25 .. 2^25 with full mantissas, and rows at the edges
     of the magnitude range the bound is stated for
  f  exclusion ranges against segments, stages and poison rows
  g  pools smaller than a stage, at the one / two segment edge, and users with
     exactly P, P + 1 and P + 2 candidates

Every comparison is bit for bit against the CPU oracle composition of
tests/test_gpu_lsh_closest.py (oracle_expect). Every case the screen takes also
asserts settled + lists == nq and that the counter `seen` is the sum of the
oracle's list lengths (the kernel counts a candidate before it looks at
whether its user is still alive, so handed-back users count too). Each case's
preconditions are asserted from the oracle alone, before the GPU runs.
Data are data26 (26-bit values) unless stated."""
import functools

import numpy as np
import pytest

import oracle
from amd import lshkm
from test_gpu_lsh_closest import (assert_same, bits, build_cosine, ctx, data26, main_shape,  # noqa: F401 (ctx: fixture)
                                  oracle_expect, oracle_lists, run, ties_shape)

pytestmark = pytest.mark.gpu
SEED = 12345        # build_cosine's projection seed


def expect_of(X, U, lists, P):
    """oracle_expect's composition over lists computed once (shared by a ladder's cases)."""
    cp = np.cumsum([0] + [len(c) for c in lists]).astype(np.int64)
    ci = np.concatenate(list(lists) + [np.zeros(0, np.int32)]).astype(np.int32)
    w_idx, w_sim, w_cnt = oracle.p_closest(X, U, cp, ci, P)
    return w_idx, w_sim, w_cnt, np.diff(cp), (cp, ci)


def screen_run(mod, c, X, U, k, L, P, want, excl=None, route="screen", label=""):
    """One call on a fresh index: outputs and counters, checked against `want`."""
    nq = U.shape[0]
    lsh, Xd, _ = build_cosine(mod, c, X, k, L, SEED)
    try:
        got, st = run(mod, c, lsh, Xd, U, P, excl)
    finally:
        lsh.close()
    print(f"{label}: settled {st[0]} lists {st[1]} kept {st[2]} seen {st[3]} "
          f"candidates/user {want[3].min()}..{want[3].max()}")
    assert_same(got, want)
    if route == "lists":
        assert st == (0, nq, 0, 0)
    else:
        assert st[0] + st[1] == nq
        assert st[3] == int(want[3].sum()), "seen is not the sum of the users' list lengths"
    return got, st


# ------------------------------------------------- a. the capacity ladder
LADDER_P = [95, 96, 223, 224, 300, 447, 448]


@functools.lru_cache(maxsize=None)
def ladder_pool(N):
    """N = 2000: one segment, 457..689 candidates per user (a list passes 448
    entries inside the walk); N = 6000: five segments of 1216 rows, none with
    448 candidates of one user. Data seed 17. Also every user's first 449
    similarities: finite and strictly decreasing here, so for every P of the
    ladder the first P + 1 are (they are the P + 1 largest of a list without
    ties among its first 449)."""
    X, U = data26(17, N, 130, 100)
    R, _ = oracle.gen_lsh_cosine(SEED, 5, 4, 100)
    lists = oracle_lists(X, U, R)
    first = expect_of(X, U, lists, max(LADDER_P) + 1)[1]
    return X, U, tuple(lists), first


@pytest.mark.parametrize("N", [2000, 6000])
@pytest.mark.parametrize("P", LADDER_P)
def test_capacity_ladder(ctx, sw, sctx, monkeypatch, P, N):
    """Measured on an MI355X (users handed back = overflows, the precondition
    leaves no other reason): product capacity, none up to P = 300 on either
    pool and none at N = 6000; 18 of 130 at N = 2000, P = 447, where cap ==
    cap_min. Smallest capacity (P = 95 / 223 / 447): 46 / 53 / 18 at N = 2000,
    89 / 50 / 0 at N = 6000. The counts are printed, not asserted: they follow
    from the f32 intervals, the outputs do not."""
    X, U, lists, first = ladder_pool(N)
    want = expect_of(X, U, lists, P)
    # preconditions, as test_main_shape's: only an overflow may hand a user back
    assert want[3].min() > P + 1
    assert np.isfinite(first[:, :P + 1]).all()
    assert (np.diff(first[:, :P + 1], axis=1) < 0).all(), "two of a user's first P + 1 similarities are equal"
    assert np.array_equal(bits(first[:, :P]), bits(want[1]))
    got, st = screen_run(lshkm, ctx, X, U, 4, 5, P, want, route="lists" if P == 448 else "screen",
                         label=f"capacity ladder N={N} P={P}")
    if P <= 447:
        assert st[0] > 0, "every user went through the lists path"
    if P in (95, 223, 447):
        monkeypatch.setenv("LSHKM_LSHPC_CAP", "small")
        try:
            got_s, _ = screen_run(sw, sctx, X, U, 4, 5, P, want, label=f"capacity ladder N={N} P={P} small capacity")
        finally:
            monkeypatch.delenv("LSHKM_LSHPC_CAP", raising=False)
        assert_same(got_s, got)


# ------------------------------------------------- b. the code-width ladder
def only_in_table(X, U, R, t):
    """(user, row) pairs that share a bucket in table t and in no other."""
    eq = oracle.lsh_hash_cosine(U, R)[:, None, :] == oracle.lsh_hash_cosine(X, R)[None, :, :]
    others = np.delete(eq, t, axis=2).any(axis=2)
    return int((eq[:, :, t] & ~others).sum())


@pytest.mark.parametrize("k,L,N,P,own", [
    (8, 4, 6000, 20, False),        # 64..169 candidates per user
    (4, 8, 1061, 20, False),        # 355..500
    (2, 16, 1061, 20, False),       # 1038..1057
    (16, 2, 6000, 5, True),         # U = X[:130]: each user has at least itself
    (11, 3, 6000, 20, False),       # 33 bits: the lists path
])
def test_code_width(ctx, k, L, N, P, own):
    X, U = data26(17, N, 130, 100)
    if own:
        U = X[:130].copy()
    R, _ = oracle.gen_lsh_cosine(SEED, L, k, 100)
    want = oracle_expect(X, U, R, P)
    if L * k == 32:
        # the top field ends at bit 31 and the lowest starts at bit 0: both must decide alone
        last, low = only_in_table(X, U, R, L - 1), only_in_table(X, U, R, 0)
        print(f"pairs sharing a bucket only in table {L - 1}: {last}, only in table 0: {low}")
        assert last > 0 and low > 0
    if own:
        assert want[3].min() >= 1
    _, st = screen_run(lshkm, ctx, X, U, k, L, P, want, route="screen" if L * k <= 32 else "lists",
                       label=f"code width k={k} L={L}")
    if L * k <= 32:
        assert st[0] > 0


# ------------------------------------------------- c. the dimension ladder
@pytest.mark.parametrize("d", [1, 2, 31, 32, 33, 127, 128, 129])
def test_dimensions(ctx, d):
    N, nq, k, L, P = 1061, 130, 4, 5, 20
    X, U = data26(17, N, nq, d)
    R, _ = oracle.gen_lsh_cosine(SEED, L, k, d)
    want = oracle_expect(X, U, R, P)
    assert want[3].min() > P + 1
    _, st = screen_run(lshkm, ctx, X, U, k, L, P, want, route="lists" if d == 129 else "screen",
                       label=f"dimensions d={d}")
    if d == 1:
        # every similarity is +-1: ties, which only the lists path orders
        assert np.isin(want[1], (-1.0, 1.0)).all()
        assert st[1] > 0


# ------------------------------------------------- d. user chunks
def poison_chunks(nq, zero_users):
    """test_poison's rows; the zero users at `zero_users`."""
    X, U = data26(17, 1061, nq, 100)
    X[10] = 0.0
    X[20, 3] = np.inf
    X[30] *= 1e200
    X[40] *= 1e-200
    for q in zero_users:
        U[q] = 0.0
    return X, U


@functools.lru_cache(maxsize=None)
def chunk_case(name):
    """(X, U, k, L, P, excl, want). Chunks of 128 users: main 4 x 128 + 88, ties
    128 + 72 (replay users in the second chunk), poison 128 + 2 with both zero
    users in the ragged last chunk and 2 x 128 + 44 with one in the middle chunk
    and one in the last, exclusion 128 + 2."""
    if name == "main":
        X, U, R, want = main_shape(False)
        return X, U, 4, 5, 20, None, want
    if name == "ties":
        X, U, R, want = ties_shape()
        return X, U, 4, 5, 15, None, want
    excl = None
    if name == "poison130":
        X, U = poison_chunks(130, (128, 129))
    elif name == "poison300":
        X, U = poison_chunks(300, (130, 299))
    else:
        assert name == "exclusion"
        X, U = data26(17, 1061, 130, 100)
        excl = (200, 517)
    R, _ = oracle.gen_lsh_cosine(SEED, 5, 4, 100)
    return X, U, 4, 5, 20, excl, oracle_expect(X, U, R, 20, excl)


@pytest.mark.parametrize("name", ["main", "ties", "poison130", "poison300", "exclusion"])
def test_user_chunks(sw, sctx, monkeypatch, name):
    X, U, k, L, P, excl, want = chunk_case(name)
    nq = U.shape[0]
    assert nq > 128, "one chunk only"
    if name == "ties":
        # users the settle must replay (a tie among the first P + 1) in the second chunk
        w16 = oracle.p_closest(X, U, want[4][0], want[4][1], P + 1)[1]
        tied = (np.diff(w16, axis=1) == 0).any(axis=1) & (want[3] > P + 1)
        assert tied[128:].any() and tied[:128].any()
    if name.startswith("poison"):
        lists = oracle_lists(X, U, oracle.gen_lsh_cosine(SEED, L, k, 100)[0])
        has = np.array([np.isin([10, 20, 30, 40], c).any() for c in lists])
        assert has[:128].any() and (~has[:128]).any() and (~(U != 0).any(axis=1))[128:].any()
    lsh, Xd, _ = build_cosine(sw, sctx, X, k, L, SEED)
    try:
        plain, st_p = run(sw, sctx, lsh, Xd, U, P, excl)
        monkeypatch.setenv("LSHKM_LSHPC_BUDGET", "small")
        chunked, st_c = run(sw, sctx, lsh, Xd, U, P, excl)
        again, st_a = run(sw, sctx, lsh, Xd, U, P, excl) if name == "main" else (chunked, st_c)
    finally:
        monkeypatch.delenv("LSHKM_LSHPC_BUDGET", raising=False)
        lsh.close()
    print(f"user chunks {name}: one chunk {st_p} chunks of 128 {st_c}")
    assert_same(plain, want)
    assert_same(chunked, want)
    assert_same(again, want)
    assert st_c == st_p, "the counters depend on the chunking"
    assert st_a == st_c, "counters differ between two runs of the same call"
    assert st_c[0] + st_c[1] == nq
    assert st_c[3] == int(want[3].sum())
    if name in ("ties", "poison130", "poison300"):
        assert st_c[1] > 0
    if name != "ties":                # there every user has a tie among its first P + 1
        assert st_c[0] > 0


# ------------------------------------------------- e. magnitudes, full mantissas
@functools.lru_cache(maxsize=None)
def magnitude_case():
    """N = 2000, nq = 130, d = 100, data seed 23: standard_normal rows and users,
    each times a uniform [1, 2) factor and 2^e, e an integer of [-25, 25] drawn
    per row: sums of squares within about 2^+-59. Then four rows rescaled by a
    power of two to sums of squares in (2^62, 2^64], (2^64, 2^66), [2^-64,
    2^-62) and (2^-66, 2^-64): two at the range's edges inside, two outside."""
    rng = np.random.default_rng(23)
    N, nq, d = 2000, 130, 100

    def draw(n):
        A = rng.standard_normal((n, d))
        return A * rng.uniform(1.0, 2.0, size=(n, 1)) * np.exp2(rng.integers(-25, 26, size=(n, 1)).astype(np.float64))

    X, U = draw(N), draw(nq)
    planted = {}
    for row, (lo, hi) in zip((100, 700, 1300, 1900), ((62, 64), (64, 66), (-64, -62), (-66, -64))):
        e = np.log2(np.sum(X[row] * X[row]))
        m = int(np.floor(((lo + hi) / 2 - e) / 2 + 0.5))      # x * 2^m: the sum of squares times 4^m (exact)
        X[row] = X[row] * np.exp2(float(m))
        e = np.log2(np.sum(X[row] * X[row]))
        assert lo + 0.01 < e < hi - 0.01, (row, e)            # clear of the edge by far more than a summation order
        planted[row] = e
    R, _ = oracle.gen_lsh_cosine(SEED, 5, 4, d)
    lists = oracle_lists(X, U, R)
    want = expect_of(X, U, lists, 20)
    return X, U, tuple(lists), want, planted


def test_magnitudes(ctx):
    X, U, lists, want, planted = magnitude_case()
    nq, P = 130, 20
    ss = np.sum(X * X, axis=1)
    out = np.nonzero((ss > 2.0 ** 64) | (ss < 2.0 ** -64))[0]
    assert sorted(out) == [700, 1900] and sorted(planted) == [100, 700, 1300, 1900]
    ssu = np.sum(U * U, axis=1)
    assert ssu.min() >= 2.0 ** -64 and ssu.max() <= 2.0 ** 64
    # the doubles are full-mantissa ones: the conversion to f32 loses bits in nearly every value
    assert (X.astype(np.float32).astype(np.float64) != X).mean() > 0.99
    has_out = np.array([np.isin(out, c).any() for c in lists])
    has_edge = np.array([np.isin([100, 1300], c).any() for c in lists])
    print(f"users with an out-of-range candidate {has_out.sum()}, with an in-range edge row {has_edge.sum()}")
    assert (~has_out).sum() > nq // 2, "more than half of the users have only in-range candidates"
    assert has_out.any() and (has_edge & ~has_out).any()
    assert want[3].min() > P + 1
    _, st = screen_run(lshkm, ctx, X, U, 4, 5, P, want, label="magnitudes")
    assert st[1] >= has_out.sum()
    assert st[0] > 0


# ------------------------------------------------- f. exclusion, poison, segments
@functools.lru_cache(maxsize=None)
def segment_pool():
    """N = 6000, nq = 130: five segments of 1216 rows (lshpc_plan: at least 1024 rows each)."""
    X, U = data26(17, 6000, 130, 100)
    R, _ = oracle.gen_lsh_cosine(SEED, 5, 4, 100)
    return X, U, R


@pytest.mark.parametrize("excl", [(1216, 2432), (1215, 1281), (0, 6000)])
def test_exclusion_segments(ctx, excl):
    X, U, R = segment_pool()
    P = 20
    want = oracle_expect(X, U, R, P, excl)
    got, st = screen_run(lshkm, ctx, X, U, 4, 5, P, want, excl, label=f"exclusion {excl}")
    assert ((got[0] < excl[0]) | (got[0] >= excl[1])).all()
    if excl == (0, 6000):
        assert (got[3] == 0).all() and (got[2] == 0).all() and (got[0] == -1).all() and (bits(got[1]) == 0).all()
        assert st[3] == 0
    else:
        assert want[3].min() > P + 1 and st[0] > 0


def test_excluded_poison(ctx):
    X0, U, R = segment_pool()
    P, excl = 20, (1216, 2432)
    X = X0.copy()
    X[1220] = 0.0                    # test_poison's four rows, all inside the excluded segment
    X[1279, 3] = np.inf              # the last row of a stage
    X[1280] *= 1e200                 # the first row of the next
    X[2431] *= 1e-200                # the segment's last row
    assert (U != 0).any(axis=1).all(), "no poison user"
    want0 = oracle_expect(X0, U, R, P, excl)
    want = oracle_expect(X, U, R, P, excl)
    # rows the exclusion drops change no list (the poison rows hash elsewhere, that is all)
    assert np.array_equal(want[3], want0[3]) and np.array_equal(want[0], want0[0])
    assert np.isfinite(want[1]).all()
    _, st0 = screen_run(lshkm, ctx, X0, U, 4, 5, P, want0, excl, label="excluded segment, no poison")
    _, st = screen_run(lshkm, ctx, X, U, 4, 5, P, want, excl, label="excluded segment with the poison rows in it")
    assert st == st0, "an excluded poison row flagged a user"
    assert st[0] > 0


# ------------------------------------------------- g. small pools, the P + 1 edge
@pytest.mark.parametrize("nq", [127, 128, 129])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 2047, 2048, 2049])
def test_small_pools(ctx, N, nq):
    k, L, d, P = 2, 2, 8, 5
    X, U = data26(17, N, nq, d)
    R, _ = oracle.gen_lsh_cosine(SEED, L, k, d)
    want = oracle_expect(X, U, R, P)
    if N == 1:
        assert (want[3] == 0).any() and (want[3] == 1).any(), "fewer candidates than P: none, and one"
    else:
        assert want[3].min() >= 1 and want[3].max() > P + 1
    got, _ = screen_run(lshkm, ctx, X, U, k, L, P, want, label=f"small pool N={N} nq={nq}")
    pad = np.arange(P)[None, :] >= got[2][:, None]
    assert (got[0][pad] == -1).all() and (bits(got[1])[pad] == 0).all()


P_EDGE_SEED = 17      # data seed of the P + 1 edge case (chosen on the CPU)


def test_p_plus_one_edge(ctx):
    N, nq, d, P, k, L = 1061, 130, 7, 5, 8, 2
    X, U = data26(P_EDGE_SEED, N, nq, d)
    R, _ = oracle.gen_lsh_cosine(SEED, L, k, d)
    want = oracle_expect(X, U, R, P)
    # the last step prunes a list iff it holds more than P + 1 entries
    for n in (P, P + 1, P + 2):
        assert (want[3] == n).any(), f"no user with exactly {n} candidates"
    screen_run(lshkm, ctx, X, U, k, L, P, want, label="P + 1 edge")
