"""GPU parity: lshkm_min_vector_dist and its lists form (DESIGN.md §5f;
csrc/nearest_layout.h is the rule, csrc/nearest.hip the kernels,
csrc/api_nearest.cpp the entry points).

Expectations: the fixtures of tests/golden/nearest (the reference's own
min_vector_euclidean_dist / min_vector_cosine_dist) and, for the larger cases,
oracle.lloyd_assign(Q, X, metric), which tests/test_nearest_cpu.py pins to the
fixtures bit for bit: its distance is the helper's value, its argmin the first
row attaining it. Everything is compared bit for bit."""
import functools

import numpy as np
import pytest

import oracle
from amd import lshkm
from nearest_cases import FIXTURES, first_row, fixture, fixture_is_f32

pytestmark = pytest.mark.gpu
S_SETTLED, S_SCAN, S_EXACT = lshkm.STAT_NEAREST_SETTLED, lshkm.STAT_NEAREST_SCAN, lshkm.STAT_NEAREST_EXACT
SWITCHES = ("LSHKM_NEAREST_PATH", "LSHKM_NEAREST_CAP", "LSHKM_NEAREST_SEG")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def dev(c, a):
    return c.torch.from_numpy(np.ascontiguousarray(a)).to(c.dev)


def run(mod, c, X, Q, metric):
    """One call: (dist, row) on the host and the three counters' deltas."""
    before = [c.stat(s) for s in (S_SETTLED, S_SCAN, S_EXACT)]
    dist, row = mod.min_vector_dist(c, dev(c, X), dev(c, Q), metric)
    c.sync()
    st = tuple(c.stat(s) - b for s, b in zip((S_SETTLED, S_SCAN, S_EXACT), before))
    return dist.cpu().numpy(), row.cpu().numpy(), st


def assert_same(got, want_dist, want_row, label=""):
    d, r = got[0], got[1]
    bad = np.nonzero(bits(d) != bits(want_dist))[0]
    assert bad.size == 0, f"{label}: dist differs at queries {bad[:8]}: {d[bad[:4]]} vs {want_dist[bad[:4]]}"
    bad = np.nonzero(r != want_row)[0]
    assert bad.size == 0, f"{label}: row differs at queries {bad[:8]}: {r[bad[:4]]} vs {want_row[bad[:4]]}"


def all_paths(c, sw, sctx, monkeypatch, X, Q, metric, want_dist, want_row, label):
    """Product = exact-forced = screen-forced = smallest-capacity = small-segments,
    each against the expectation (so also against one another). Returns the
    counters of each."""
    out = {}
    got = run(lshkm, c, X, Q, metric)
    assert_same(got, want_dist, want_row, f"{label} product")
    out["product"] = got[2]
    for name, env in (("exact", {"LSHKM_NEAREST_PATH": "exact"}), ("screen", {"LSHKM_NEAREST_PATH": "screen"}),
                      ("cap", {"LSHKM_NEAREST_CAP": "small"}), ("seg", {"LSHKM_NEAREST_SEG": "small"}),
                      ("cap+seg", {"LSHKM_NEAREST_CAP": "small", "LSHKM_NEAREST_SEG": "small"})):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            g = run(sw, sctx, X, Q, metric)
        finally:
            for k in SWITCHES:
                monkeypatch.delenv(k, raising=False)
        assert_same(g, want_dist, want_row, f"{label} {name}")
        out[name] = g[2]
    nq = Q.shape[0] if X.shape[0] else 0          # N == 0: no query is screened or scanned
    assert out["exact"] == (0, nq, 0), out["exact"]
    for name, st in out.items():
        print(f"{label} {name}: settled {st[0]} scan {st[1]} exact distances {st[2]}")
        assert st[0] + st[1] == nq
    return out


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(ctx, sw, sctx, monkeypatch, name):
    x, q, metric, dist = fixture(name)
    rows = first_row(x, q, metric, dist)
    if x.shape[0] == 0:
        assert not dist.any() and (rows == -1).all()
    all_paths(ctx, sw, sctx, monkeypatch, x, q, metric, dist, rows, name)
    if fixture_is_f32(name):
        all_paths(ctx, sw, sctx, monkeypatch, x.astype(np.float32), q.astype(np.float32), metric, dist, rows,
                  name + " fp32")


# ------------------------------------------------------ oracle-composed cases
def normal_rows(seed, n, d, f32):
    a = np.random.default_rng(seed).standard_normal((n, d))
    return a.astype(np.float32) if f32 else a


# every N, nq and d once, and the corners: (N, nq, d)
SHAPES = [(1, 1, 1), (63, 127, 20), (64, 129, 32), (65, 1, 33), (4097, 127, 128), (4097, 129, 129), (63, 1, 300),
          (4097, 129, 1), (1, 129, 128), (4097, 1, 300), (64, 127, 129), (65, 129, 20)]


@pytest.mark.parametrize("f32", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("N,nq,d", SHAPES)
def test_oracle_shapes(ctx, sw, sctx, monkeypatch, N, nq, d, metric, f32):
    """One LDS stage (63 / 64 / 65 rows), one query tile (127 / 129), both dp
    instantiations (32 / 33), the d > 128 route (128 / 129 / 300)."""
    X = normal_rows(100 + N + d, N, d, f32)
    Q = normal_rows(200 + nq + d, nq, d, f32)
    Q[::3] = X[(np.arange(0, nq, 3) * 7) % N]                 # a third of the queries are rows: distance 0 (or its rounding)
    wa, wd = oracle.lloyd_assign(Q, X, metric)
    st = all_paths(ctx, sw, sctx, monkeypatch, X, Q, metric, wd, wa, f"N={N} nq={nq} d={d} {metric}")
    if d > 128:
        assert st["product"] == (0, nq, 0), "d > 128 is the exact scan's"
    elif d > 1:          # d = 1 under cosine: every distance is 0 or 2, half the rows tie
        assert st["product"][1] == 0 and st["screen"][1] == 0, "a clean call sent queries to the scan"


# ---------------------------------------------------------------- hard inputs
def test_every_row_twice(ctx, sw, sctx, monkeypatch):
    """The answer is the lower index of each pair."""
    for metric in ("euclidean", "cosine"):
        X = np.repeat(normal_rows(5, 500, 24, False), 2, axis=0)
        Q = normal_rows(6, 96, 24, False)
        Q[::2] = X[(np.arange(0, 96, 2) * 13) % 1000]
        wa, wd = oracle.lloyd_assign(Q, X, metric)
        assert (wa % 2 == 0).all()
        st = all_paths(ctx, sw, sctx, monkeypatch, X, Q, metric, wd, wa, f"twice {metric}")
        assert st["product"][2] >= 2 * 96, "the screen cannot separate a pair: both are the settle's"


def test_one_ulp_neighbours(ctx, sw, sctx, monkeypatch):
    """Rows that differ from a query's true neighbour in one coordinate by one
    ulp: the screen cannot separate them, the settle must."""
    for metric in ("euclidean", "cosine"):
        rng = np.random.default_rng(9)
        base = rng.standard_normal((200, 16))
        Q = base[:64] + rng.standard_normal((64, 16)) * 2.0 ** -6
        X = np.concatenate([base, base[:64], base[:64]])
        j = rng.integers(0, 16, 64)
        X[200 + np.arange(64), j] = np.nextafter(base[np.arange(64), j], np.inf)
        X[264 + np.arange(64), j] = np.nextafter(base[np.arange(64), j], -np.inf)
        X = X[rng.permutation(X.shape[0])]
        wa, wd = oracle.lloyd_assign(Q, X, metric)
        st = all_paths(ctx, sw, sctx, monkeypatch, X, Q, metric, wd, wa, f"one ulp {metric}")
        assert st["product"][2] >= 3 * 64


def test_cancellation(ctx, sw, sctx, monkeypatch):
    """All rows 1000 + 2^-10 noise (euclidean): |q|^2 + |x|^2 is 2^31 times the
    squared distances, the intervals are wide and every row stays possible."""
    rng = np.random.default_rng(11)
    X = 1000.0 + rng.standard_normal((700, 12)) * 2.0 ** -10
    Q = 1000.0 + rng.standard_normal((40, 12)) * 2.0 ** -10
    wa, wd = oracle.lloyd_assign(Q, X, "euclidean")
    st = all_paths(ctx, sw, sctx, monkeypatch, X, Q, "euclidean", wd, wa, "cancellation")
    assert st["cap"][1] > 0, "the smallest capacity did not overflow"


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("at0", [True, False], ids=["row0", "elsewhere"])
def test_poison(ctx, sw, sctx, monkeypatch, metric, at0):
    """Three poison rows among 1,000 (an inf entry, a 1e200 entry, a zero row
    under cosine / an all-1e-200 row under euclidean), at row 0 (the NaN rule
    decides) or elsewhere, and two poison queries. The other queries are the
    screen's: the poison rows join their kept rows."""
    rng = np.random.default_rng(13)
    X = rng.standard_normal((1000, 20))
    Q = rng.standard_normal((70, 20))
    p = [0, 1, 2] if at0 else [333, 640, 999]
    zero = 0 if at0 else 1                   # cosine: the zero row at row 0 makes every result its NaN
    X[p[zero]] = 0.0 if metric == "cosine" else 1e-200
    X[p[1 - zero]][3] = np.inf
    X[p[2]][5] = -1e200
    Q[7][3] = np.inf                         # inf - inf against the inf row
    Q[21] = 0.0 if metric == "cosine" else 1e-200
    wa, wd = oracle.lloyd_assign(Q, X, metric)
    if at0 and metric == "cosine":
        assert np.isnan(wd).all() and (wa == 0).all()
    st = all_paths(ctx, sw, sctx, monkeypatch, X, Q, metric, wd, wa, f"poison {metric} at0={at0}")
    assert st["product"][1] == 2, "only the two poison queries are the scan's"
    assert st["product"][2] >= 3 * 68, "the poison rows were not settled for every query"


def test_too_many_poison_rows(ctx):
    """More poison rows than the settle takes on: the call is the scan's."""
    X = normal_rows(15, 300, 8, False)
    X[::10, 2] = np.inf
    Q = normal_rows(16, 9, 8, False)
    wa, wd = oracle.lloyd_assign(Q, X, "euclidean")
    got = run(lshkm, ctx, X, Q, "euclidean")
    assert_same(got, wd, wa, "30 poison rows")
    assert got[2] == (0, 9, 0)


def test_workspace_reuse(ctx):
    """A small, a larger and again the small shape on one context."""
    small = (normal_rows(17, 100, 8, False), normal_rows(18, 5, 8, False))
    large = (normal_rows(19, 3000, 100, False), normal_rows(20, 300, 100, False))
    for X, Q in (small, large, small):
        for metric in ("euclidean", "cosine"):
            wa, wd = oracle.lloyd_assign(Q, X, metric)
            assert_same(run(lshkm, ctx, X, Q, metric), wd, wa, f"reuse N={X.shape[0]} {metric}")


def test_both_dist_modes(ctx, dist_mode):
    """The exact chain in both modes of the context."""
    X, Q = normal_rows(21, 500, 20, True), normal_rows(22, 50, 20, True)
    wa, wd = oracle.lloyd_assign(Q, X, "euclidean")
    assert_same(run(lshkm, ctx, X, Q, "euclidean"), wd, wa, dist_mode)


# ------------------------------------------------------- clean-case condition
@functools.lru_cache(maxsize=None)
def clean_case(which):
    if which == "normal128":
        rng = np.random.default_rng(1)
        X, Q = rng.standard_normal((5000, 128)), rng.standard_normal((300, 128))
    else:                                    # k / 64 grid scores in [-1, 3) at d = 17
        rng = np.random.default_rng(1)
        X, Q = rng.integers(-64, 192, (5000, 17)) / 64.0, rng.integers(-64, 192, (300, 17)) / 64.0
    return X, Q


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("which", ["normal128", "grid17"])
def test_clean_case(ctx, which, metric):
    """No query to the scan and at most 4 exact distances per query on average."""
    X, Q = clean_case(which)
    wa, wd = oracle.lloyd_assign(Q, X, metric)
    got = run(lshkm, ctx, X, Q, metric)
    assert_same(got, wd, wa, f"clean {which} {metric}")
    print(f"clean {which} {metric}: settled {got[2][0]} scan {got[2][1]} exact distances {got[2][2]} "
          f"({got[2][2] / 300:.3f} per query)")
    assert got[2][1] == 0
    assert got[2][0] == 300
    assert got[2][2] <= 4 * 300


# ----------------------------------------------------------------- lists form
def lists_expect(X, Q, metric, ptr, idx):
    dist = np.zeros(Q.shape[0])
    row = np.full(Q.shape[0], -1, np.int32)
    for q in range(Q.shape[0]):
        li = idx[ptr[q]:ptr[q + 1]]
        if li.size:
            a, d = oracle.lloyd_assign(Q[q:q + 1], X[li], metric)
            dist[q], row[q] = d[0], li[a[0]]
    return dist, row


def run_lists(c, X, Q, metric, ptr, idx):
    d, r = lshkm.min_vector_dist_lists(c, dev(c, X), dev(c, Q), metric, dev(c, ptr.astype(np.int64)),
                                       dev(c, idx.astype(np.int32)))
    c.sync()
    return d.cpu().numpy(), r.cpu().numpy()


@functools.lru_cache(maxsize=None)
def index_data():
    rng = np.random.default_rng(23)
    X = (rng.integers(-64, 192, (2000, 32)) / 64.0)
    Q = X[rng.integers(0, 2000, 150)] + rng.integers(-8, 9, (150, 32)) / 64.0
    return X, Q


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_lists_from_lsh(ctx, metric):
    X, Q = index_data()
    R, _ = lshkm.params_lsh_cosine(12345, 3, 6, 32)
    lsh = lshkm.LSH(ctx, "cosine", 32, 6, 3, R=R)
    try:
        Xd = dev(ctx, X)
        lsh.build(Xd)
        ptr, idx = lsh.query(dev(ctx, Q), filtered=True, device=True)
        d, r = lshkm.min_vector_dist_lists(ctx, Xd, dev(ctx, Q), metric, ptr, idx)
        ctx.sync()
        wd, wr = lists_expect(X, Q, metric, ptr.cpu().numpy(), idx.cpu().numpy())
        assert (np.diff(ptr.cpu().numpy()) > 0).sum() > 100
        assert_same((d.cpu().numpy(), r.cpu().numpy()), wd, wr, f"lsh lists {metric}")
    finally:
        lsh.close()


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_lists_from_cube(ctx, metric):
    X, Q = index_data()
    R, _ = lshkm.params_cube_cosine(12345, 7, 32)
    cube = lshkm.Cube(ctx, "cosine", 32, 7, R=R)
    try:
        Xd = dev(ctx, X)
        cube.build(Xd)
        ptr, idx = cube.query(dev(ctx, Q), 5, device=True)
        d, r = lshkm.min_vector_dist_lists(ctx, Xd, dev(ctx, Q), metric, ptr, idx)
        ctx.sync()
        wd, wr = lists_expect(X, Q, metric, ptr.cpu().numpy(), idx.cpu().numpy())
        assert_same((d.cpu().numpy(), r.cpu().numpy()), wd, wr, f"cube lists {metric}")
    finally:
        cube.close()


def test_lists_edges(ctx):
    """An empty list, a list of one, an unsorted list with a tie (first in list
    wins), a list that starts with a NaN row (the NaN rule is the list's), one
    that holds it later."""
    X = normal_rows(29, 50, 6, False)
    X[20] = X[10]
    X[30] = 0.0                               # cosine: NaN
    Q = np.stack([X[10] + 0.01, X[3], X[10] + 0.01, X[5], X[5]])
    lists = [[], [7], [40, 20, 4, 10, 49], [30, 5, 6], [6, 30, 5]]
    ptr = np.cumsum([0] + [len(li) for li in lists])
    idx = np.array(sum(lists, []), np.int32)
    for metric in ("euclidean", "cosine"):
        wd, wr = lists_expect(X, Q, metric, ptr, idx)
        assert wd[0] == 0.0 and wr[0] == -1 and wr[1] == 7 and wr[2] == 20
        if metric == "cosine":
            assert np.isnan(wd[3]) and wr[3] == 30 and wr[4] == 5
        assert_same(run_lists(ctx, X, Q, metric, ptr, idx), wd, wr, f"lists edges {metric}")
        assert_same(run_lists(ctx, X.astype(np.float32), Q.astype(np.float32), metric, ptr, idx),
                    *lists_expect(X.astype(np.float32), Q.astype(np.float32), metric, ptr, idx), f"lists edges fp32 {metric}")


def test_lists_bad_index(ctx):
    X, Q = normal_rows(31, 10, 4, False), normal_rows(32, 2, 4, False)
    for idx in ([1, 2, 10], [1, -1, 3]):
        with pytest.raises(lshkm.LshkmError, match="lshkm error -1"):
            run_lists(ctx, X, Q, "euclidean", np.array([0, 2, 3]), np.array(idx))
    with pytest.raises(lshkm.LshkmError, match="lshkm error -1"):
        run_lists(ctx, X, Q, "euclidean", np.array([0, 3, 2]), np.array([1, 2, 3]))
    assert_same(run_lists(ctx, X, Q, "euclidean", np.array([0, 2, 3]), np.array([1, 2, 9])),
                *lists_expect(X, Q, "euclidean", np.array([0, 2, 3]), np.array([1, 2, 9])), "after the errors")


# -------------------------------------------------------------- index_quality
@pytest.mark.parametrize("kind", ["lsh", "cube"])
def test_index_quality(ctx, kind):
    X, Q = index_data()
    Xd, Qd = dev(ctx, X), dev(ctx, Q)
    if kind == "lsh":
        R, _ = lshkm.params_lsh_cosine(777, 2, 7, 32)
        index = lshkm.LSH(ctx, "cosine", 32, 7, 2, R=R)
    else:
        R, _ = lshkm.params_cube_cosine(777, 8, 32)
        index = lshkm.Cube(ctx, "cosine", 32, 8, R=R)
    try:
        index.build(Xd)
        ptr, idx = (index.query(Qd, filtered=True) if kind == "lsh" else index.query(Qd, 3))
        got = lshkm.index_quality(ctx, index, Xd, Qd, "cosine", probes=3)
    finally:
        index.close()
    bd, br = lists_expect(X, Q, "cosine", ptr, idx)
    ta, td = oracle.lloyd_assign(Q, X, "cosine")
    has = br >= 0
    pos = has & (td > 0)
    ratio = bd[pos] / td[pos]
    assert 0 < has.sum() and 0 < pos.sum()
    assert got["found"] == has.sum() / 150 and got["recall_at_1"] == (has & (bd == td)).sum() / 150
    assert got["ratio_mean"] == pytest.approx(ratio.mean(), rel=1e-12) and got["ratio_max"] == pytest.approx(ratio.max(), rel=1e-12)
    assert_same((got["bucket_dist"].cpu().numpy(), got["bucket_row"].cpu().numpy()), bd, br, "bucket")
    assert_same((got["true_dist"].cpu().numpy(), got["true_row"].cpu().numpy()), td, ta, "true")


# ------------------------------------------------------------ argument errors
def test_argument_errors(ctx):
    import ctypes as C
    t = ctx.torch
    X = t.zeros((4, 3), dtype=t.float64, device=ctx.dev)
    Q = t.zeros((2, 3), dtype=t.float64, device=ctx.dev)
    dist = ctx.empty((2,), t.float64)
    row = ctx.empty((2,), t.int32)
    ptr = t.zeros((3,), dtype=t.int64, device=ctx.dev)
    p = lambda a: C.c_void_p(a.data_ptr())
    f, fl = lshkm.lib().lshkm_min_vector_dist_f64, lshkm.lib().lshkm_min_vector_dist_lists_f64
    assert f(ctx.h, p(X), 4, 0, p(Q), 2, 0, p(dist), p(row)) == -1            # d = 0
    assert f(ctx.h, p(X), 4, 3, p(Q), 2, 2, p(dist), p(row)) == -1            # unknown metric
    assert f(ctx.h, p(X), 4, 3, p(Q), 2, 0, None, p(row)) == -1               # null output
    assert f(ctx.h, None, 4, 3, p(Q), 2, 0, p(dist), p(row)) == -1
    assert f(ctx.h, p(X), 4, 3, None, 2, 0, p(dist), p(row)) == -1
    assert f(ctx.h, p(X), -1, 3, p(Q), 2, 0, p(dist), p(row)) == -1
    assert f(ctx.h, p(X), 1 << 31, 3, p(Q), 2, 0, p(dist), p(row)) == -1
    assert f(None, p(X), 4, 3, p(Q), 2, 0, p(dist), p(row)) == -1
    assert fl(ctx.h, p(X), 4, 0, p(Q), 2, 0, p(ptr), None, p(dist), p(row)) == -1
    assert fl(ctx.h, p(X), 4, 3, p(Q), 2, 0, None, None, p(dist), p(row)) == -1
    assert fl(ctx.h, p(X), 4, 3, p(Q), 2, 0, p(ptr), None, None, p(row)) == -1
    assert f(ctx.h, p(X), 4, 3, p(Q), 0, 0, None, None) == 0                  # nq == 0: nothing to do
    assert f(ctx.h, p(X), 4, 3, p(Q), 2, 0, p(dist), None) == 0               # rows are optional
    assert fl(ctx.h, p(X), 4, 3, p(Q), 2, 0, p(ptr), None, p(dist), p(row)) == 0      # all lists empty
    ctx.sync()
    assert not dist.cpu().numpy().any() and (row.cpu().numpy() == -1).all()
