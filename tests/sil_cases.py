"""Inputs for the silhouette's structural edges (csrc/silhouette.hip,
csrc/pairsum.h and the grid test of csrc/update.hip), and plain restatements
used to check that each case reaches the branch it is meant for. CPU only:
numpy (and the C oracle's row generator), no GPU import.

case(label) -> (X, assign, C, metric, label). The expectations of the GPU
tests come from oracle.silhouette alone; tests/test_sil_cases_cpu.py asserts on
the host the property that makes each case mean something (which cluster is
whose nearest, where the NaNs fall, that pow(x, 2) and x*x part), with the
restatements below (dist_np, near_np, sil_np), which share no code with the
oracle.

Families:
  planted  the cluster sizes of test_gpu_pam.SIZES around the 64-member batch of
           sil_segment, a singleton, an empty cluster that is cluster 3's
           nearest; over a table of d / row type / metric / value kind
  kedge    K = 1, 2, 65, 257, 300, duplicate centroids, zero centroids (cosine)
  value    inf, squares that overflow or land in the subnormal range, -0.0
  agrid    grid rows with one off-grid value at the first or last element of X
Fixtures of tests/golden/sil (the reference's own results; make_golden.py
--only sil) are read with fixture(); fixture_inputs() builds their inputs."""
import functools
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "sil")
DEFAULT_NAN = 0xFFF8000000000000          # x86's 0/0

SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 129, 257, 0]      # test_gpu_pam.SIZES; cluster 11 is empty


# ------------------------------------------------------------------ pieces
def sizes_assign(sizes, seed):
    """Per-row cluster ids: cluster c owns sizes[c] rows at shuffled positions,
    so the cluster-sorted row list is not the identity."""
    a = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(sizes)])
    return np.random.RandomState(seed).permutation(a)


def gen_rows(kind, d, N, dtype, seed, zero_every=0):
    """test_gpu_pam.gen_rows: "grid" (multiples of 2^-15 below 4), "normal"
    (full fp32 mantissas), "wide" (a grid wider than 26 bits in one column),
    "general" (fp64 only: doubles with no fp32 image)."""
    import oracle
    X = oracle.synth(seed, N, d, kind="grid" if kind in ("grid", "wide") else "normal")
    if kind == "wide":
        X[::7, min(3, d - 1)] *= np.float32(2.0 ** 12)
    X = X.astype(dtype)
    if kind == "general":
        assert np.dtype(dtype) == np.float64
        X = X * (1.0 + 2.0 ** -30) + 2.0 ** -40
    if zero_every:
        X[::zero_every] = 0.0
    return X


def first_members(X, assign, K):
    """C[c] = the fp64 image of cluster c's first member (zeros if it has none)."""
    C = np.zeros((K, X.shape[1]))
    for c in range(K):
        mem = np.nonzero(assign == c)[0]
        if len(mem):
            C[c] = X[mem[0]].astype(np.float64)
    return C


def nudge(c):
    return c * (1.0 + 2.0 ** -10) + 2.0 ** -12


def _tag(dtype, metric):
    return ("f32" if np.dtype(dtype) == np.float32 else "f64") + "-" + ("eu" if metric == "euclidean" else "cos")


# ------------------------------------------------------------------ planted
# d, dtype, metric, kind, zero_every, odd variant too, assignment seed (None: d).
# d = 1 under cosine: every distance is 0 or 2 (the sign), so near[3] == 11
# needs the first members of clusters 1, 2, 4..10 on the other side of zero
# from cluster 3's, and the singleton's row a cluster-1 member on the other
# side of its own (else b = 0 and s = 0/0); 6699 is the first shuffle seed that
# does both.
PLANTED_TABLE = [
    (1, np.float32, "euclidean", "grid", 0, False, None),
    (1, np.float64, "cosine", "general", 0, False, 6699),
    (2, np.float32, "euclidean", "normal", 0, False, None),
    (3, np.float32, "euclidean", "normal", 0, True, None),
    (5, np.float64, "euclidean", "grid", 0, False, None),
    (7, np.float32, "euclidean", "wide", 0, False, None),
    (4, np.float32, "euclidean", "grid", 0, True, None),
    (12, np.float64, "euclidean", "general", 0, False, None),
    (100, np.float32, "euclidean", "normal", 0, False, None),
    (33, np.float32, "cosine", "normal", 101, False, 35),      # the singleton stays clear of the zero rows
    (33, np.float64, "euclidean", "general", 0, False, None),
    (511, np.float32, "euclidean", "grid", 0, False, None),
    (512, np.float32, "euclidean", "normal", 0, False, None),
    (512, np.float64, "euclidean", "general", 0, False, None),
    (513, np.float32, "euclidean", "grid", 0, True, None),
    (513, np.float64, "cosine", "general", 0, True, None),
    (600, np.float32, "euclidean", "wide", 0, False, None),
]


def planted_sizes(odd):
    s = list(SIZES)
    if odd:
        s[10] = 256                       # N = 679: the last wave has no second member
    return s


def planted(d, dtype, metric, kind, zero_every=0, odd=False, seed=None):
    sizes = planted_sizes(odd)
    N, K = sum(sizes), len(sizes)
    assign = sizes_assign(sizes, (d if seed is None else seed) + (5000 if odd else 0))
    X = gen_rows(kind, d, N, dtype, 800 + d, zero_every)
    C = first_members(X, assign, K)
    C[11] = nudge(C[3])                   # the empty cluster: cluster 3's nearest, b = 0/0
    C[0] = nudge(C[4])                    # the singleton: cluster 4's nearest
    return X, assign, C, metric


def _planted_label(d, dtype, metric, kind, odd):
    return f"planted-d{d}-{_tag(dtype, metric)}-{kind}" + ("-odd" if odd else "")


PLANTED = {}
for (_d, _dt, _m, _k, _z, _odd, _s) in PLANTED_TABLE:
    for _o in ([False, True] if _odd else [False]):
        PLANTED[_planted_label(_d, _dt, _m, _k, _o)] = functools.partial(planted, _d, _dt, _m, _k, _z, _o, _s)


# ------------------------------------------------------------------ K edges
KEDGE_NAMES = ["k1", "k2", "k65", "k257", "k300", "dup"]
CZERO_NAMES = ["czero0", "czero1", "czerolast"]


def kedge(name, d, metric):
    seed = 900 + d + 17 * (KEDGE_NAMES + CZERO_NAMES).index(name)
    rs = np.random.RandomState(seed)
    if name == "k1":
        N, K = 151, 1                     # odd: the last wave's member is alone
        assign = np.zeros(N, np.int32)
    elif name == "k2":
        N, K = 150, 2
        assign = sizes_assign([61, 89], seed)
    elif name == "k65":
        N, K = 130, 65                    # sil_near_kernel's second block
        assign = sizes_assign([2] * 65, seed)
    elif name in ("k257", "k300"):
        N, K = 200, int(name[1:])         # K > N; sil_sum_kernel's strided loop
        assign = rs.randint(0, K, N).astype(np.int32)
        assign[0] = K - 1
    elif name == "dup":
        N, K = 160, 8
        assign = sizes_assign([20] * 8, seed)
    else:
        N, K = 140, 6
        assign = sizes_assign([20, 30, 25, 15, 40, 10], seed)
    X = gen_rows("normal", d, N, np.float32, seed)
    C = first_members(X, assign, K)
    if name in ("k257", "k300"):
        # empty clusters: far from the data, except every 10th, which stays
        # among it (somebody's nearest: b = 0/0)
        E = gen_rows("normal", d, K, np.float32, seed + 1).astype(np.float64)
        for c in range(K):
            if not (assign == c).any():
                C[c] = E[c] + (0.0 if c % 10 == 0 else 64.0)
    if name == "dup":
        C[5] = C[2]
        C[6] = C[0]
        C[7] = C[0]
    if name in CZERO_NAMES:
        C[{"czero0": 0, "czero1": 1, "czerolast": K - 1}[name]] = 0.0
    return X, assign, C, metric


KEDGES = {}
for _n in KEDGE_NAMES:
    for (_d, _m) in [(7, "euclidean"), (8, "euclidean"), (7, "cosine")]:
        KEDGES[f"kedge-{_n}-d{_d}-{'eu' if _m == 'euclidean' else 'cos'}"] = functools.partial(kedge, _n, _d, _m)
for _n in CZERO_NAMES:
    for _d in (7, 8):
        KEDGES[f"kedge-{_n}-d{_d}-cos"] = functools.partial(kedge, _n, _d, "cosine")


# ------------------------------------------------------------------ hard values
VALUE_NAMES = ["inf", "huge", "tiny520", "tiny300", "negzero"]
VALUE_SIZES = [50, 50, 50, 51]


def value_case(name, d, scale_up=False):
    """N = 201, K = 4. The special values sit in members 3, 10 and 20 of one
    cluster, never in a first member (the centroids stay ordinary): the cluster
    that is the nearest of the fewest others, so that at least two clusters keep
    finite silhouettes."""
    seed = 950 + d
    assign = sizes_assign(VALUE_SIZES, seed)
    N = len(assign)
    metric = "cosine" if name == "negzero" else "euclidean"
    if name in ("inf", "negzero"):
        X = gen_rows("normal" if name == "inf" else "grid", d, N, np.float32, seed)
    else:
        X = gen_rows("general", d, N, np.float64, seed)
    near = near_np(first_members(X, assign, 4), metric)
    h = int(np.argmin(np.bincount(near, minlength=4)))
    mem = np.nonzero(assign == h)[0]
    if name == "inf":
        X[mem[3], 2] = X[mem[10], 2] = np.inf
        X[mem[20], 2] = -np.inf
    elif name == "huge":
        X[mem[3], 1], X[mem[10], 1], X[mem[20], 4] = 1e200, -1e200, 1e200
    elif name in ("tiny520", "tiny300"):
        if name == "tiny300":
            # two clusters 2^-225 below the others, each the other's nearest:
            # their squares land in the subnormal range, the others' near 2^-600
            lo = [c for c in range(4) if c != h][:2]
            X[np.isin(assign, lo)] *= 2.0 ** -225
        X = np.ldexp(X, -int(name[4:]) + (520 if scale_up else 0))
    else:
        X[::5, 1] = -0.0
        X[1::9, d - 1] = -0.0
        X[mem[3]] = X[mem[10]] = -0.0     # zero rows of negative zeros: NaN cosine distances
    C = first_members(X, assign, 4)
    return X, assign, C, metric


VALUES = {f"value-{n}-d{d}": functools.partial(value_case, n, d) for n in VALUE_NAMES for d in (6, 8)}
# grid rows with -0.0 entries under euclidean: the grid test must read them as zeros
VALUES["value-negzero-grid-d6"] = lambda: _negzero_grid(6)
VALUES["value-negzero-grid-d8"] = lambda: _negzero_grid(8)


def _negzero_grid(d):
    X, assign, _, _ = value_case("negzero", d)
    X[X.sum(axis=1) == 0] = np.float32(0.5)      # no zero rows here
    X[0, 0] = X[-1, -1] = -0.0
    return X, assign, first_members(X, assign, 4), "euclidean"


def value_scaled_up(label):
    """The tiny case `label` times 2^520 (rows and centroids): no square underflows."""
    _, name, dd = label.split("-")
    return value_case(name, int(dd[1:]), scale_up=True)


# ------------------------------------------------------------------ almost-grid
AGRID_SIZES = [40, 41, 3]                 # N = 84: N * d is no multiple of 64 for d = 2, 5


def pow2(x):
    """libm's pow(x, 2), as the reference calls it."""
    try:
        return math.pow(x, 2.0)
    except OverflowError:
        return math.inf


def mul2(x):
    return x * x


@functools.lru_cache(maxsize=None)
def _hard_doubles():
    """Doubles in [1, 2) whose pow(x, 2) is not x*x, by the midpoint filter of
    tests/test_gpu_pow2.py::inputs (Dekker's exact x*x = p + e)."""
    rng = np.random.default_rng(11)
    x = rng.uniform(1.0, 2.0, 400000)
    p = x * x
    c = 134217729.0 * x
    xh = c - (c - x)
    xl = x - xh
    e = ((xh * xh - p) + 2.0 * xh * xl) + xl * xl
    u = np.ldexp(1.0, np.frexp(p)[1] - 53)
    near = np.abs(np.abs(e) - 0.5 * u) <= u * 2.0 ** -8
    return [float(v) for v in x[near] if pow2(float(v)) != float(v) * float(v)]


AGRID_MATES = 8


def _grid_dists(Y):
    """[N][N] euclidean distances of grid rows: every square is exact, so numpy's
    x*x is pow(x, 2); the adds run in coordinate order as the reference's."""
    Y = Y.astype(np.float64)
    acc = np.zeros((len(Y), len(Y)))
    for k in range(Y.shape[1]):
        df = Y[:, k][:, None] - Y[:, k][None, :]
        acc = acc + df * df
    return np.sqrt(acc)


def _s_from_dists(D, assign, near):
    """s [N] from a distance matrix: the sums in member order, vectorised over rows."""
    K = len(near)
    mem = [np.nonzero(assign == c)[0] for c in range(K)]
    s = np.empty(len(assign))
    for c in range(K):
        a = np.zeros(len(mem[c]))
        for j in mem[c]:
            a = a + D[mem[c], j]
        if len(mem[c]) != 1:
            a = a / (len(mem[c]) - 1)
        b = np.zeros(len(mem[c]))
        for j in mem[near[c]]:
            b = b + D[mem[c], j]
        b = b / len(mem[near[c]])
        s[mem[c]] = (b - a) / np.where(b > a, b, a)
    return s


def almost_grid(dtype, d, where, grid_only=False):
    """Grid rows (multiples of 2^-15 below 4) with one off-grid value at element
    0 (where = "first") or N * d - 1 ("last") of X. The value and the same
    coordinate of AGRID_MATES cluster mates are chosen by search, until the
    silhouettes computed with pow(x, 2) differ in bits from those with x*x:
      fp64: x from _hard_doubles (53 bits), the mates' coordinate 0.0, so the
            difference is x itself (then, if none of them shows, small grid values);
      fp32: x an odd multiple of 2^-26 below 2^-3 and the mates' coordinate g a
            grid value with 1.5 <= |x - g| < 2: the difference has 27 significant
            bits, its square 54: an exact tie, which pow rounds by its own error
            and x*x to even.
    Only distances from the off-grid row can differ (all other squares are
    exact), so the search fills that row of an otherwise exact distance matrix.
    grid_only: the same matrix with a grid value in place of the off-grid one."""
    f32 = np.dtype(dtype) == np.float32
    assign = sizes_assign(AGRID_SIZES, 40 + d)
    N = len(assign)
    r, j = (0, 0) if where == "first" else (N - 1, d - 1)
    assert (assign == assign[r]).sum() >= 40, "choose a seed that puts the row in a large cluster"
    X = gen_rows("grid", d, N, dtype, 990 + d)
    mates = [m for m in np.nonzero(assign == assign[r])[0] if m != r][:AGRID_MATES]
    rng = np.random.default_rng(5 + d + (0 if where == "first" else 100))
    grid = [-1.5, -1.75, 1.75, -1.5 - 2.0 ** -15, 1.875, -1.625]      # |x - g| in [1.5, 2): the square has 54 bits
    found = None
    for t in range(3000):
        if f32:
            x = float(2 * int(rng.integers(0, 1 << 22)) + 1) * 2.0 ** -26
            g = [grid[int(i)] for i in rng.integers(0, len(grid), len(mates))]
        else:
            x = _hard_doubles()[t % len(_hard_doubles())]
            g = [0.0] * len(mates) if t < len(_hard_doubles()) else [float(rng.integers(-4, 5)) * 0.25 for _ in mates]
        Y = X.copy()
        Y[r, j] = x
        for m, gv in zip(mates, g):
            Y[m, j] = gv
        near = near_np(first_members(Y, assign, 3), "euclidean")
        Dp = _grid_dists(Y)
        Dm = Dp.copy()
        for i in range(N):
            Dp[r, i] = Dp[i, r] = dist_np(Y[r], Y[i], "euclidean", pow2)
            Dm[r, i] = Dm[i, r] = dist_np(Y[r], Y[i], "euclidean", mul2)
        sp, sm = _s_from_dists(Dp, assign, near), _s_from_dists(Dm, assign, near)
        if not np.array_equal(sp.view(np.uint64), sm.view(np.uint64)):
            found = Y
            break
    assert found is not None, "no off-grid value found"
    X = found
    assert X.dtype == np.dtype(dtype)
    if grid_only:
        X = X.copy()
        X[r, j] = 0.5
    return X, assign, first_members(X, assign, 3), "euclidean"


AGRID = {f"agrid-{'f32' if dt == np.float32 else 'f64'}-d{d}-{w}": functools.partial(almost_grid, dt, d, w)
         for dt in (np.float64, np.float32) for d in (2, 5) for w in ("first", "last")}


def almost_grid_base(label):
    """The all-grid matrix of an almost-grid case (same context before and after)."""
    return AGRID[label](grid_only=True) + (label + "-base",)


# ------------------------------------------------------------------ access
CASES = {}
for _g in (PLANTED, KEDGES, VALUES, AGRID):
    CASES.update(_g)


@functools.lru_cache(maxsize=None)
def _case(label):
    X, assign, C, metric = CASES[label]()
    X = np.ascontiguousarray(X)
    for a in (X, assign, C):
        a.setflags(write=False)
    return X, assign, C, metric, label


def case(label):
    """(X [N][d] fp32 or fp64, assign [N] int32, C [K][d] fp64, metric name, label);
    built once, read-only."""
    return _case(label)


# ------------------------------------------------------------------ restatements
def dist_np(a, b, metric, sq=pow2):
    """The reference's distance of two fp64 vectors (cust_vector.hpp:124-155),
    term by term: squares by `sq`, sequential adds, the cosine's inner product
    in x87 long double."""
    a = [float(v) for v in a]
    b = [float(v) for v in b]
    with np.errstate(all="ignore"):
        if metric == "euclidean":
            acc = np.float64(0.0)
            for u, v in zip(a, b):
                acc = acc + np.float64(sq(float(np.float64(u) - np.float64(v))))
            return float(np.sqrt(acc))
        ip = np.longdouble(0.0)
        x = y = np.float64(0.0)
        for u, v in zip(a, b):
            ip = ip + np.longdouble(np.float64(u) * np.float64(v))
            x, y = x + np.float64(sq(u)), y + np.float64(sq(v))
        denom = np.sqrt(x) * np.sqrt(y)
        return float(1.0 - np.float64(ip / np.longdouble(denom)))


def near_np(C, metric):
    """silhouette.hpp:35-58: the -1 sentinel, strict <."""
    K = len(C)
    near = np.zeros(K, np.int32)
    for c in range(K):
        mn, arg = -1.0, 0
        for i in range(K):
            if i == c:
                continue
            dd = dist_np(C[c], C[i], metric)
            if mn == -1 or dd < mn:
                mn, arg = dd, i
        near[c] = arg
    return near


def sil_np(X, assign, C, metric, sq=pow2):
    """silhouette_cluster restated (small N only): s [N] with squares by `sq`."""
    X64 = np.asarray(X).astype(np.float64)
    K = len(C)
    near = near_np(C, metric)
    mem = [np.nonzero(assign == c)[0] for c in range(K)]
    s = np.empty(len(X64))
    with np.errstate(all="ignore"):
        for c in range(K):
            for r in mem[c]:
                a = np.float64(0.0)
                for j in mem[c]:
                    a = a + np.float64(dist_np(X64[r], X64[j], metric, sq))
                if len(mem[c]) != 1:
                    a = a / np.float64(len(mem[c]) - 1)
                b = np.float64(0.0)
                for j in mem[near[c]]:
                    b = b + np.float64(dist_np(X64[r], X64[j], metric, sq))
                b = b / np.float64(len(mem[near[c]]))
                mx = b if b > a else a
                s[r] = (b - a) / mx
    return s


def grid_rule(X):
    """grid_exact_squares restated (csrc/update.hip): every finite nonzero value
    is a multiple of 2^q below 2^t with t - q <= 25 and q >= -460, and none is
    inf or nan."""
    import km_shard_np as ksn
    x = np.asarray(X, np.float64).ravel()
    if not np.isfinite(x).all():
        return False
    x = x[x != 0.0]
    if x.size == 0:
        return True
    q, t = ksn.bit_positions(x)
    return bool(t.max() - q.min() <= 25 and q.min() >= -460)


def straddles(assign):
    """(pairs whose two members lie in two clusters, pairs within one cluster)
    among the pairs (p, p + 1), p even, of the cluster-sorted order."""
    sa = np.sort(assign, kind="stable")
    n = len(sa) // 2
    diff = sa[0:2 * n:2] != sa[1:2 * n:2]
    return int(diff.sum()), int((~diff).sum())


# ------------------------------------------------------------------ fixtures
FIXTURE_KINDS = ["k1", "k2", "planted", "dup", "czero_first", "czero_mid", "czero_rows", "inf"]
FIXTURE_NAMES = [f"sil_{k}_d{d}" for k in FIXTURE_KINDS for d in (3, 8)]
FIXTURE_SIZES = [1, 2, 3, 33, 65, 0]      # the planted construction, shrunk


def fixture_inputs(name):
    """(x [N][d] fp64, assign, C, metric name) of a tests/golden/sil fixture:
    N <= 200; d = 3: fp32 values, d = 8: general doubles."""
    kind, d = name[4:name.rindex("_")], int(name[name.rindex("_") + 2:])
    seed = 970 + d + 7 * FIXTURE_KINDS.index(kind)
    gen = lambda N: (gen_rows("normal", d, N, np.float32, seed).astype(np.float64) if d == 3
                     else gen_rows("general", d, N, np.float64, seed))
    metric = "cosine" if kind.startswith("czero") else "euclidean"
    if kind == "k1":
        X, assign = gen(91), np.zeros(91, np.int32)
    elif kind == "k2":
        X, assign = gen(120), sizes_assign([47, 73], seed)
    elif kind == "planted":
        assign = sizes_assign(FIXTURE_SIZES, seed)
        X = gen(len(assign))
    elif kind == "dup":
        X, assign = gen(160), sizes_assign([20] * 8, seed)
    elif kind == "czero_rows":
        X, assign = gen(150), sizes_assign([30, 50, 45, 25], seed)
        near = near_np(first_members(X, assign, 4), "cosine")
        mem = np.nonzero(assign == int(np.argmin(np.bincount(near, minlength=4))))[0]
        X[mem[3]] = X[mem[10]] = X[mem[20]] = 0.0     # in the cluster fewest others are nearest to
    elif kind == "inf":
        X, assign = gen(150), sizes_assign([40, 40, 35, 35], seed)
        mem = np.nonzero(assign == 0)[0]
        X[mem[3], 2] = X[mem[10], 2] = np.inf
        X[mem[20], 2] = -np.inf
    else:
        X, assign = gen(140), sizes_assign([20, 30, 25, 15, 40, 10], seed)
    K = int(assign.max()) + 1 if kind != "planted" else len(FIXTURE_SIZES)
    C = first_members(X, assign, K)
    if kind == "planted":
        C[5] = nudge(C[3])
        C[0] = nudge(C[4])
    if kind == "dup":
        C[5] = C[2]
        C[6] = C[0]
        C[7] = C[0]
    if kind == "czero_first":
        C[0] = 0.0
    if kind == "czero_mid":
        C[3] = 0.0
    return np.ascontiguousarray(X), assign.astype(np.int32), C, metric


def fixtures():
    return sorted(f[:-4] for f in os.listdir(DIR) if f.endswith(".npz")) if os.path.isdir(DIR) else []


def fixture(name):
    """(x fp64, assign, C, metric name, sil [K+1], s [N]: the reference's)."""
    g = np.load(os.path.join(DIR, name + ".npz"))
    return g["x"], g["assign"], g["centers"], "cosine" if int(g["metric"][0]) else "euclidean", g["sil"], g["s"]
