"""Host checks of tests/sil_cases.py: the oracle runs on every case, and each
case has the property that makes it mean something on the GPU
(tests/test_gpu_silhouette_edges.py) -- which cluster is whose nearest, where
the NaNs fall, that the rows pass or fail the grid rule, that pow(x, 2) and
x*x part. The properties are recomputed with sil_cases' plain restatements
(near_np, sil_np), not read from the oracle's internals."""
import numpy as np
import pytest

import km_shard_np as ksn
import oracle
import sil_cases as sc


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


_ORACLE = {}


def oracle_of(label):
    if label not in _ORACLE:
        X, assign, C, metric, _ = sc.case(label)
        _ORACLE[label] = oracle.silhouette(X, assign, C, metric)
    return _ORACLE[label]


@pytest.mark.parametrize("label", list(sc.CASES))
def test_oracle_runs(label):
    X, assign, C, metric, _ = sc.case(label)
    out, s = oracle_of(label)
    N, K = len(assign), len(C)
    assert out.shape == (K + 1,) and s.shape == (N,)
    assert X.shape[0] == N and C.shape[1] == X.shape[1] and assign.dtype == np.int32
    assert assign.min() >= 0 and assign.max() < K
    # every NaN the oracle gives is x86's default NaN
    for v in (out, s):
        assert np.all(bits(v)[np.isnan(v)] == sc.DEFAULT_NAN)
    # empty clusters are 0/0
    cnt = np.bincount(assign, minlength=K)
    assert np.all(bits(out[:K])[cnt == 0] == sc.DEFAULT_NAN)


def test_table_is_the_issue():
    got = sorted((d, "f32" if dt == np.float32 else "f64", m, k) for (d, dt, m, k, _, _, _) in sc.PLANTED_TABLE)
    want = sorted([(1, "f32", "euclidean", "grid"), (1, "f64", "cosine", "general"), (2, "f32", "euclidean", "normal"),
                   (3, "f32", "euclidean", "normal"), (5, "f64", "euclidean", "grid"), (7, "f32", "euclidean", "wide"),
                   (4, "f32", "euclidean", "grid"), (12, "f64", "euclidean", "general"),
                   (100, "f32", "euclidean", "normal"), (33, "f32", "cosine", "normal"),
                   (33, "f64", "euclidean", "general"), (511, "f32", "euclidean", "grid"),
                   (512, "f32", "euclidean", "normal"), (512, "f64", "euclidean", "general"),
                   (513, "f32", "euclidean", "grid"), (513, "f64", "cosine", "general"),
                   (600, "f32", "euclidean", "wide")])
    assert got == want
    odd = sorted(l for l in sc.PLANTED if l.endswith("-odd"))
    assert [l.split("-")[1] for l in odd] == ["d3", "d4", "d513", "d513"], odd


# ------------------------------------------------------------------ planted
@pytest.mark.parametrize("label", list(sc.PLANTED))
def test_planted_preconditions(label):
    X, assign, C, metric, _ = sc.case(label)
    out, s = oracle_of(label)
    odd = label.endswith("-odd")
    cnt = np.bincount(assign, minlength=12)
    assert list(cnt) == sc.planted_sizes(odd) and len(assign) == (679 if odd else 680)
    assert not np.array_equal(np.argsort(assign, kind="stable"), np.arange(len(assign)))      # rows[] is not the identity
    near = sc.near_np(C, metric)
    assert near[3] == 11, near                  # a nonempty cluster whose nearest is empty: b = 0/0
    assert near[4] == 0, near                   # the singleton is somebody's nearest
    assert np.isnan(out[3]) and np.isnan(out[11])
    assert np.all(np.isnan(s[assign == 3]))
    single = int(np.nonzero(assign == 0)[0][0])
    assert np.isfinite(s[single]), s[single]    # a is not divided: 0 / 0 would be NaN
    two, one = sc.straddles(assign)
    assert two >= 1 and one >= 1, (two, one)
    if "-grid" in label:
        assert sc.grid_rule(X)
    else:
        assert not sc.grid_rule(X)
    if "-cos-normal" in label:                  # zero rows, one of them leading its cluster
        zero = np.nonzero(~X.any(axis=1))[0]
        assert len(zero) == 7
        assert any(z == np.nonzero(assign == assign[z])[0][0] for z in zero)
    if "-general" in label:
        assert not np.array_equal(X.astype(np.float32).astype(np.float64), X)


# ------------------------------------------------------------------ K edges
@pytest.mark.parametrize("label", list(sc.KEDGES))
def test_kedge_preconditions(label):
    X, assign, C, metric, _ = sc.case(label)
    out, s = oracle_of(label)
    N, K = len(assign), len(C)
    assert 130 <= N <= 300
    name = label.split("-")[1]
    cnt = np.bincount(assign, minlength=K)
    if name == "k1":
        assert K == 1 and N % 2 == 1 and np.isfinite(s).all()
    elif name == "k2":
        assert K == 2 and cnt.min() > 0
    elif name == "k65":
        assert K == 65 and N == 130 and np.all(cnt == 2)
    elif name in ("k257", "k300"):
        assert K == int(name[1:]) and N == 200 and K > N
        assert np.isnan(s).any() and np.isfinite(s).sum() >= N // 2
        assert (cnt[256:] > 0).any()            # a member beyond sil_sum_kernel's first stride
    elif name == "dup":
        assert bits(C[2]).tolist() == bits(C[5]).tolist()
        assert bits(C[0]).tolist() == bits(C[6]).tolist() == bits(C[7]).tolist()
        near = sc.near_np(C, metric)
        assert near[5] == 2 and near[2] == 5 and near[6] == 0 and near[7] == 0 and near[0] == 6, near
    else:
        z = {"czero0": 0, "czero1": 1, "czerolast": K - 1}[name]
        assert metric == "cosine" and not C[z].any() and C[np.arange(K) != z].any(axis=1).all()
        near = sc.near_np(C, metric)
        if name != "czerolast":
            assert near[0] == 1, near           # the NaN is visited first and sticks
        else:
            assert near[0] != K - 1 and near[K - 1] == 0, near


def test_kedges_cover_both_routes_and_cosine():
    for name in sc.KEDGE_NAMES:
        assert {f"kedge-{name}-d7-eu", f"kedge-{name}-d8-eu", f"kedge-{name}-d7-cos"} <= set(sc.KEDGES)
    for name in sc.CZERO_NAMES:
        assert {f"kedge-{name}-d7-cos", f"kedge-{name}-d8-cos"} <= set(sc.KEDGES)


# ------------------------------------------------------------------ hard values
@pytest.mark.parametrize("label", list(sc.VALUES))
def test_value_preconditions(label):
    X, assign, C, metric, _ = sc.case(label)
    out, s = oracle_of(label)
    name = label.split("-")[1]
    assert len(assign) == 201 and len(C) == 4
    if "grid" in label:
        assert np.signbit(X[X == 0]).any() and X[0, 0] == 0 and np.signbit(X[0, 0]) and np.signbit(X[-1, -1])
        assert sc.grid_rule(X) and np.isfinite(s).all()
        return
    if name in ("tiny520", "tiny300"):
        Xu, au, Cu, mu = sc.value_scaled_up(label)
        assert np.array_equal(np.ldexp(Xu, -520), X) and np.array_equal(np.ldexp(Cu, -520), C)
        _, su = oracle.silhouette(Xu, au, Cu, mu)
        # squares below 2^-1022: the silhouettes are not those of the scaled-up rows
        assert not np.array_equal(bits(s), bits(su))
        ax = np.abs(X[X != 0])
        if name == "tiny520":
            assert ax.max() < 2.0 ** -511
        else:
            # two clusters near 2^-525 (each the other's nearest), the rest near
            # 2^-300: squares near 2^-600, outside gp_sq_slow's [2^-40, 2^40)
            # window, and squares in the subnormal range, in one matrix. (A
            # plain 2^-300 scaling cannot differ from its scaled-up image: a
            # power of two scales every operation of the reference exactly.)
            assert (ax < 2.0 ** -511).any() and (ax > 2.0 ** -310).any() and ax.max() < 2.0 ** -290
            moved = bits(s) != bits(su)
            lo = np.unique(assign[(np.abs(X) < 2.0 ** -500).all(axis=1)])
            assert len(lo) == 2 and np.isin(assign[moved], lo).all()
        return
    assert np.isnan(s).any() and np.isfinite(s).any(), (np.isnan(s).sum(), np.isfinite(s).sum())
    if name == "inf":
        col = X[:, 2]
        assert X.dtype == np.float32 and (col == np.inf).sum() == 2 and (col == -np.inf).sum() == 1
        assert np.isfinite(np.delete(X, 2, axis=1)).all()
    elif name == "huge":
        assert X.dtype == np.float64 and (np.abs(X) == 1e200).sum() == 3
    else:
        assert np.signbit(X[X == 0]).any() and (~X.any(axis=1)).sum() == 2


# ------------------------------------------------------------------ almost-grid
@pytest.mark.parametrize("label", list(sc.AGRID))
def test_almost_grid_preconditions(label):
    X, assign, C, metric, _ = sc.case(label)
    Xg, ag, Cg, mg, _ = sc.almost_grid_base(label)
    _, s = oracle_of(label)
    N, d = X.shape
    assert N == 84 and sorted(np.bincount(assign)) == [3, 40, 41] and (N * d) % 64 != 0
    assert metric == "euclidean" and np.array_equal(ag, assign)
    # one element differs, the first or the last of X; without it the rows are a grid
    diff = np.nonzero(X.ravel() != Xg.ravel())[0]
    assert list(diff) == [0 if label.endswith("first") else N * d - 1]
    assert sc.grid_rule(Xg) and not sc.grid_rule(X)
    # some difference of the off-grid value and a cluster mate's has more than 26 significant bits
    r, j = (0, 0) if label.endswith("first") else (N - 1, d - 1)
    col = X[assign == assign[r], j].astype(np.float64)
    df = float(X[r, j]) - col[col != float(X[r, j])]
    q, t = ksn.bit_positions(df)
    assert (t - q > 26).any()
    # the silhouettes tell pow(x, 2) from x*x: an EXSQ kernel on these rows gives other bits
    s_pow = sc.sil_np(X, assign, C, metric, sc.pow2)
    s_mul = sc.sil_np(X, assign, C, metric, sc.mul2)
    assert np.array_equal(bits(s_pow), bits(s))             # the restatement is the oracle's silhouette
    ndiff = int((bits(s_pow) != bits(s_mul)).sum())
    assert ndiff >= 1, ndiff
    # on the all-grid rows the two agree (every square is exact)
    assert np.array_equal(bits(sc.sil_np(Xg, ag, Cg, mg, sc.pow2)), bits(sc.sil_np(Xg, ag, Cg, mg, sc.mul2)))


def test_fixture_inputs_are_small():
    for name in sc.FIXTURE_NAMES:
        X, assign, C, metric = sc.fixture_inputs(name)
        assert X.dtype == np.float64 and X.shape[0] <= 200 and X.shape[1] in (3, 8)
        assert len(assign) == X.shape[0] and C.shape[1] == X.shape[1]


@pytest.mark.parametrize("name", sc.FIXTURE_NAMES)
def test_fixture_preconditions(name):
    """The reference's own results (tests/golden/sil) do sit at the edge each
    fixture is named for."""
    x, assign, C, metric, sil, s = sc.fixture(name)
    xi, ai, Ci, mi = sc.fixture_inputs(name)
    assert np.array_equal(bits(x), bits(xi)) and np.array_equal(assign, ai) and np.array_equal(bits(C), bits(Ci)) and metric == mi
    kind = name[4:name.rindex("_")]
    K = len(C)
    cnt = np.bincount(assign, minlength=K)
    near = sc.near_np(C, metric)
    if kind == "k1":
        assert K == 1 and np.isfinite(s).all() and np.isfinite(sil).all()
    elif kind == "k2":
        assert K == 2 and list(near) == [1, 0]
    elif kind == "planted":
        assert list(cnt) == sc.FIXTURE_SIZES and near[3] == 5 and near[4] == 0
        assert np.isnan(sil[3]) and np.isnan(sil[5]) and np.isfinite(s[assign == 0]).all()
    elif kind == "dup":
        assert near[5] == 2 and near[2] == 5 and near[6] == 0 and near[7] == 0 and near[0] == 6, near
    elif kind == "czero_first":
        assert not C[0].any() and near[0] == 1 and (near[1:] == 0).all(), near     # visited first, the NaN sticks
    elif kind == "czero_mid":
        assert not C[3].any() and near[3] == 0 and (np.delete(near, 3) != 3).all(), near
    elif kind == "czero_rows":
        assert (~x.any(axis=1)).sum() == 3 and np.isnan(s).any() and np.isfinite(s).any()
    else:
        assert np.isinf(x).sum() == 3 and np.isnan(s).any() and np.isfinite(s).any()
    for v in (sil, s):
        assert np.all(bits(v)[np.isnan(v)] == sc.DEFAULT_NAN)
