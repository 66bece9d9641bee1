"""Inputs for the structural edges of the recommend step (csrc/recom.hip:
rc_p_closest_kernel, rc_replay_kernel, rc_top_n_kernel, rc_cos_sim, lomuto_sort;
csrc/predict.h), and plain restatements used to check that each case reaches
the branch it is meant for. CPU only: numpy and the C oracle, no GPU import.

case(label) -> (X, xmean, U, umean, unk_ptr, unk_idx, cand_ptr, cand_idx, P, NTOP),
built once, read-only. The expectations of the GPU tests come from
oracle.p_closest / oracle.top_n_recom alone; tests/test_recom_cases_cpu.py
asserts on the host the property that makes each case mean something (where the
tie sits, which lane its members share, that the near tie is one, which special
value comes out), with the restatements below (cos_sim_np, lomuto_np,
p_closest_np, predicted_np), which share no code with the oracle. They are used
only on rows whose squares are exact (dyadic or 26-bit values), where pow(x, 2)
and x*x cannot part.

Families:
  len    every list length around P, the 64-lane chunk and the 512-row register
         limit, for every P of LEN_P; distinct similarities; d = 24, 1, 300
  tie    one planted equality per user (a row copied or doubled under another
         index) at a chosen pair of sorted ranks around P, the pair in one lane,
         in two lanes or at the ends of the list; all-equal lists; +0.0 / -0.0
  near   the (P+1)-th best row replaced by the P-th best times 3 or 1/3: a few
         ulps apart, seldom equal
  value  inf, NaN of either sign, squares that overflow, underflow or leave
         IpAcc's range, zero rows, on the row and on the user side
  grid   launch geometry: tiny lists for more users than one sweep of the grid
  topn   (topn_case) neighbour lists written by hand for get_top_N_recom alone
Fixtures of tests/golden/recom (the reference's own results; make_golden.py
--only recomedge) are read with fixture(); fixture_inputs() builds their inputs."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "recom")
DEFAULT_NAN = 0xFFF8000000000000          # x86's "real indefinite" (0/0, inf - inf, inf * 0)
INPUT_NAN = 0x7FF8000000000000            # np.nan as an input: propagates with its own sign
NEG_ZERO = 0x8000000000000000

LEN_N = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 514, 577, 1025]      # and P-1, P, P+1, P+2
LEN_P = [1, 2, 20, 63, 64, 65, 511, 512, 600]
REG_MAX = 512                             # 64 * RC_MAXV: longer lists stream


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def csr(lists, dtype=np.int32):
    ptr = np.cumsum([0] + [len(l) for l in lists]).astype(np.int64)
    idx = np.concatenate([np.asarray(l, dtype) for l in lists]).astype(dtype) if len(lists) else np.zeros(0, dtype)
    return ptr, idx


def rows26(rng, n, d):
    """26-bit values in (-1, 1): squares are exact, products carry 52 bits."""
    return rng.integers(-2 ** 25, 2 ** 25, size=(n, d)).astype(np.float64) / 2.0 ** 25


def rows_dy(rng, n, d):
    """Multiples of 1/8 up to 5: every square and product is exact."""
    return rng.integers(-40, 41, size=(n, d)).astype(np.float64) / 8.0


def means_unknowns(rng, N, nq, d, max_m=None):
    """Dyadic means and a random ascending unknown-index list per user."""
    xm = rng.integers(-32, 33, size=N).astype(np.float64) / 16.0
    um = rng.integers(-32, 33, size=nq).astype(np.float64) / 16.0
    hi = d if max_m is None else min(d, max_m)
    unk = [np.sort(rng.choice(d, size=int(rng.integers(0, hi + 1)), replace=False)).astype(np.int32) for _ in range(nq)]
    return xm, um, unk


def pack(X, xm, U, um, unk, cand, P, NT):
    up, ui = csr(unk)
    cp, ci = csr(cand)
    return (np.ascontiguousarray(X, np.float64), xm, np.ascontiguousarray(U, np.float64), um, up, ui, cp, ci, int(P),
            int(NT))


# ------------------------------------------------------------------ restatements
def have_x87():
    """np.longdouble is the 80-bit x87 format (the x86 hosts)."""
    return np.finfo(np.longdouble).nmant == 63


def cos_sim_np(Xc, u):
    """cosineSimilarity(row, u) (cust_vector.hpp:158-174) of every row of Xc:
    the inner product of the fp64 products in 80-bit long double, the norms as
    sequential fp64 sums of squares (x*x: exact-square rows only), the division
    in long double, then fp64."""
    assert have_x87()
    Xc = np.asarray(Xc, np.float64)
    u = np.asarray(u, np.float64)
    with np.errstate(all="ignore"):
        ip = np.zeros(len(Xc), np.longdouble)
        xa = np.zeros(len(Xc), np.float64)
        ub = np.float64(0.0)
        for j in range(Xc.shape[1]):
            ip = ip + (Xc[:, j] * u[j]).astype(np.longdouble)
            xa = xa + Xc[:, j] * Xc[:, j]
            ub = ub + u[j] * u[j]
        denom = np.sqrt(xa) * np.sqrt(ub)
        return (ip / denom.astype(np.longdouble)).astype(np.float64)


def lomuto_np(key, val):
    """parallel_quickSort (crypto_rec.hpp:234-277): Lomuto, pivot = last, '>='
    to the front; the two parts are disjoint, so a stack replaces the recursion."""
    key = [float(k) for k in key]
    val = [int(v) for v in val]
    stack = [(0, len(key) - 1)]
    while stack:
        low, high = stack.pop()
        if low >= high:
            continue
        pivot = key[high]
        i = low - 1
        for j in range(low, high):
            if key[j] >= pivot:
                i += 1
                key[i], key[j] = key[j], key[i]
                val[i], val[j] = val[j], val[i]
        key[i + 1], key[high] = key[high], key[i + 1]
        val[i + 1], val[high] = val[high], val[i + 1]
        stack.append((low, i))
        stack.append((i + 2, high))
    return np.array(key, np.float64), np.array(val, np.int32)


def p_closest_np(X, U, cp, ci, P):
    """get_P_closest (crypto_rec.hpp:213-231) from cos_sim_np and lomuto_np."""
    nq = len(U)
    idx = np.full((nq, P), -1, np.int32)
    sim = np.zeros((nq, P))
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        c = ci[cp[q]:cp[q + 1]]
        if len(c) == 0:
            continue
        k, v = lomuto_np(cos_sim_np(X[c], U[q]), c)
        n = min(P, len(c))
        idx[q, :n], sim[q, :n], cnt[q] = v[:n], k[:n], n
    return idx, sim, cnt


def predicted_np(X, xm, um, up, ui, nb_idx, nb_sim, nb_cnt):
    """get_predicted_user_sim (crypto_rec.hpp:280-302) in Python floats (IEEE
    doubles, the host's own NaN rules): one value per unknown-index entry."""
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


def top_n_np(pred, up, ui, n_top):
    """get_top_N_recom's last step (crypto_rec.hpp:318-323): the quicksort of
    the predictions and the first n_top unknown indexes, 0-padded."""
    nq = len(up) - 1
    out = np.zeros((nq, n_top), np.int32)
    for q in range(nq):
        _, v = lomuto_np(pred[up[q]:up[q + 1]], ui[up[q]:up[q + 1]])
        m = min(n_top, len(v))
        out[q, :m] = v[:m]
    return out


def ulps_apart(a, b):
    """Distance of two finite doubles in units of the last place."""
    def key(x):
        b = int(np.float64(x).view(np.int64))
        return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)
    return abs(key(a) - key(b))


# ------------------------------------------------------------------ len
def len_lengths(P):
    return sorted(set(LEN_N + [P - 1, P, P + 1, P + 2]))


def len_case(P, d):
    rng = np.random.default_rng(100 + P + 1000 * d)
    N = 1100
    X = rows26(rng, N, d)
    if d == 1:
        X[X == 0] = 0.5                   # every similarity is +1 or -1, none 0/0
    lens = len_lengths(P)
    U = rows26(rng, len(lens), d)
    if d == 1:
        U[U == 0] = 0.5
    cand = [rng.permutation(N)[:n].astype(np.int32) for n in lens]          # any order, not ascending
    xm, um, unk = means_unknowns(rng, N, len(lens), d, 24)
    return pack(X, xm, U, um, unk, cand, P, 5)


LEN = {}
for _P in LEN_P:
    LEN[f"len-P{_P}-d24"] = functools.partial(len_case, _P, 24)
for _P in (20, 512):
    for _d in (1, 300):
        LEN[f"len-P{_P}-d{_d}"] = functools.partial(len_case, _P, _d)


# ------------------------------------------------------------------ tie
TIE_P = [1, 20, 63]
TIE_BASE = 700                            # distinct base rows; each user's partner rows follow
TIE_D = 20
TIE_PLACEMENTS = ["first", "Pm1_P", "P_P1", "P1_P2", "P2_P3", "triple"]
TIE_LAYOUTS = ["lane", "lanes", "ends"]
TIE_REPS = 2


def tie_ranks(placement, P):
    """The planted sorted ranks (1-based), or None where P has no such place."""
    r = {"first": [1, 2], "Pm1_P": [P - 1, P], "P_P1": [P, P + 1], "P1_P2": [P + 1, P + 2], "P2_P3": [P + 2, P + 3],
         "triple": [P - 1, P, P + 1]}[placement]
    return r if r[0] >= 1 else None


def tie_ns(P):
    return sorted({P + 2, 65, 512, 513, 600})


def _approx_order(X, c, u):
    """The rows of list c by descending similarity (fp64; the base rows'
    similarities are far apart against its error)."""
    s = (X[c] @ u) / np.sqrt((X[c] * X[c]).sum(axis=1))
    return np.argsort(-s, kind="stable")


@functools.lru_cache(maxsize=None)
def _tie_build(P):
    import oracle
    rng = np.random.default_rng(7100 + P)
    plan = []
    for placement in TIE_PLACEMENTS:
        ranks = tie_ranks(placement, P)
        if ranks is None:
            continue
        for layout in TIE_LAYOUTS:
            for n in tie_ns(P):
                if ranks[-1] > n or (layout == "lane" and n < 65) or (layout == "ends" and len(ranks) == 3 and n < 3):
                    continue
                for rep in range(TIE_REPS):
                    plan.append((placement, layout, n, rep))
    nq = len(plan)
    N = TIE_BASE + 2 * nq
    assert N <= 1100, N
    X = np.zeros((N, TIE_D))
    X[:TIE_BASE] = rows_dy(rng, TIE_BASE, TIE_D)
    U = rows_dy(rng, nq, TIE_D)
    cand, meta = [], []
    for q, (placement, layout, n, rep) in enumerate(plan):
        ranks = tie_ranks(placement, P)
        extra = len(ranks) - 1                          # partner rows
        base = rng.permutation(TIE_BASE)[:n - extra]
        order = _approx_order(X, base, U[q])
        a = int(base[order[ranks[0] - 1]])             # the row at the first planted rank
        partners = [TIE_BASE + 2 * q + t for t in range(extra)]
        for t, p in enumerate(partners):
            # the same row under another index, or a parallel one (x 2, x 1/2): equal similarities
            X[p] = X[a] * ([1.0, 2.0] if (q + rep) % 2 == 0 else [2.0, 0.5])[t]
        # Placement (P, P + 1): arrangements are drawn until the quicksort keeps
        # the tied row that stands later in the list (it cannot for P = 1 or
        # with the pair at the ends: a largest key, and a key that is the first
        # pivot's equal at position 0, never move behind their equal).
        picky = placement == "P_P1" and P > 1 and layout != "ends"
        for attempt in range(60 if picky else 1):
            members = [a] + partners
            rng.shuffle(members)
            rest = [int(r) for r in base if int(r) != a]
            rng.shuffle(rest)
            if layout == "ends":
                pos = [0, n - 1] + ([int(rng.integers(1, n - 1))] if extra == 2 else [])
            elif layout == "lane":
                i = int(rng.integers(0, n - 64))
                pos = [i, i + 64]
                if extra == 2:
                    pos.append(i + 128 if i + 128 < n else (i + 1) % n if (i + 1) % n not in pos else (i + 2) % n)
            else:
                while True:
                    pos = [int(v) for v in rng.choice(n, size=extra + 1, replace=False)]
                    if len({v % 64 for v in pos}) == len(pos):
                        break
            lst = [None] * n
            for m, p in zip(members, pos):
                lst[p] = m
            it = iter(rest)
            lst = [v if v is not None else next(it) for v in lst]
            lst = np.array(lst, np.int32)
            if not picky:
                break
            kept = int(oracle.p_closest(X, U[q:q + 1], np.array([0, n], np.int64), lst, P)[0][0, P - 1])
            if kept != members[int(np.argmin(pos))]:
                break
        cand.append(np.array(lst, np.int32))
        meta.append(dict(placement=placement, layout=layout, n=n, ranks=ranks, members=members, pos=pos[:len(members)]))
    xm, um, unk = means_unknowns(rng, N, nq, TIE_D)
    return pack(X, xm, U, um, unk, cand, P, 4), meta


def tie_meta(label):
    """Per user of a tie-P* case: placement, layout, n, the planted sorted ranks
    (1-based), the tied rows (members) and their list positions (pos)."""
    return _tie_build(int(label.split("-P")[1]))[1]


ALLEQ_N = {1: [3, 65, 512, 513, 600], 20: [2, 22, 65, 512, 513, 600]}


def tie_alleq(P):
    """Every candidate of a list is the same row (copied, or scaled by a power
    of two) under its own index: all similarities equal, the order is Lomuto's."""
    rng = np.random.default_rng(7200 + P)
    ns = ALLEQ_N[P]
    N, d = 700, TIE_D
    X = rows_dy(rng, N, d)
    U = rows_dy(rng, len(ns), d)
    row = rows_dy(rng, 1, d)[0]
    row[0] = 1.0
    X[:600] = row[None, :] * (2.0 ** rng.integers(-6, 7, size=600))[:, None]
    cand = [rng.permutation(600)[:n].astype(np.int32) for n in ns]
    xm, um, unk = means_unknowns(rng, N, len(ns), d)
    return pack(X, xm, U, um, unk, cand, P, 4)


def tie_zero():
    """+0.0 and -0.0 side by side (d = 3): inner products of +-2^-1074 over a
    denominator of 2^1000 round to zeros of either sign, beside an exact +0.0."""
    t, h = 2.0 ** -537, 2.0 ** 500
    X = np.array([[-t, 0.0, h],           # -2^-1074 / 2^1000 -> -0.0
                  [t, 0.0, h],            # +0.0 by underflow
                  [0.0, 0.0, 1.0],        # +0.0: an exact zero inner product
                  [0.0, 1.0, 0.0],        # 1
                  [0.0, -1.0, 0.0],       # -1
                  [-t, 0.0, 2.0 * h],     # -0.0 again
                  [0.0, 1.0, 1.0]])       # 1/sqrt(2)
    u = np.array([t, h, 0.0])
    lists = [[3, 0, 1, 2, 4], [0, 1, 2, 5, 3, 4, 6], [2, 5, 1, 0], [1, 0], [0, 2], [4, 5, 0, 1, 2, 3], [6, 3, 1, 5, 4]]
    U = np.tile(u, (len(lists), 1))
    rng = np.random.default_rng(7300)
    xm, um, unk = means_unknowns(rng, len(X), len(lists), 3)
    return pack(X, xm, U, um, unk, [np.array(l, np.int32) for l in lists], 3, 2)


TIE = {f"tie-P{P}": (lambda P=P: _tie_build(P)[0]) for P in TIE_P}
TIE["tie-alleq-P1"] = functools.partial(tie_alleq, 1)
TIE["tie-alleq-P20"] = functools.partial(tie_alleq, 20)
TIE["tie-zero"] = tie_zero


# ------------------------------------------------------------------ near
NEAR_P = [1, 20, 63]
NEAR_REPS = 20
NEAR_D = 100


def near_ns(P):
    return [P + 2, 80, 512]


@functools.lru_cache(maxsize=None)
def _near_build(P):
    import oracle
    rng = np.random.default_rng(7400 + P)
    plan = [(n, rep) for n in near_ns(P) for rep in range(NEAR_REPS)]
    nq = len(plan)
    B = 1000
    N = B + nq
    # partner rows: below every base row for the even users, above for the odd
    lo = (nq + 1) // 2
    X = np.zeros((N, NEAR_D))
    X[lo:lo + B] = rows26(rng, B, NEAR_D)
    U = rows26(rng, nq, NEAR_D)
    cand, meta = [], []
    for q, (n, rep) in enumerate(plan):
        base = (lo + rng.permutation(B)[:n]).astype(np.int32)
        cp = np.array([0, n], np.int64)
        idx, _, _ = oracle.p_closest(X, U[q:q + 1], cp, base, P + 1)
        a, b = int(idx[0, P - 1]), int(idx[0, P])      # the P-th and (P+1)-th best
        p = q // 2 if q % 2 == 0 else lo + B + q // 2
        X[p] = X[a] * 3.0 if rep % 2 == 0 else X[a] / 3.0
        lst = base.copy()
        lst[np.nonzero(base == b)[0][0]] = p
        cand.append(lst)
        meta.append(dict(n=n, orig=a, copy=p, pos_orig=int(np.nonzero(lst == a)[0][0]),
                         pos_copy=int(np.nonzero(lst == p)[0][0])))
    xm, um, unk = means_unknowns(rng, N, nq, NEAR_D, 24)
    return pack(X, xm, U, um, unk, cand, P, 4), meta


def near_meta(label):
    """Per user of a near-P* case: n, the original row and its scaled copy
    (pool indexes) and their list positions."""
    return _near_build(int(label.split("-P")[1]))[1]


NEAR = {f"near-P{P}": (lambda P=P: _near_build(P)[0]) for P in NEAR_P}


# ------------------------------------------------------------------ value
VALUE_ROWS = ["pinf", "ninf", "bothinf", "pnan", "nnan", "e200", "em200", "p450", "m450", "m537", "zero", "plain"]
VALUE_USERS = ["plain", "e200", "p450", "m450", "em200", "zero", "zerocol"]
VALUE_D = 12
VALUE_COL = 5                             # the column of the single inf / NaN entries


def value_case(n):
    """Row r of VALUE_ROWS is pool row r (each from its own ordinary row); the
    rows from 12 on are ordinary. Every user lists all twelve, padded with
    ordinary rows to n; P = n keeps them all. User "zerocol" is ordinary with a
    zero in column VALUE_COL: inf * 0 there, and NaN * 0."""
    rng = np.random.default_rng(7500)
    d, c = VALUE_D, VALUE_COL
    N = 700
    X = rows26(rng, N, d)
    X[X == 0] = 0.25
    U = rows26(rng, len(VALUE_USERS), d)
    U[U == 0] = 0.25
    U[:, c] = np.abs(U[:, c])
    U[:, c + 1] = np.abs(U[:, c + 1])
    k = VALUE_ROWS.index
    X[k("pinf"), c] = np.inf
    X[k("ninf"), c] = -np.inf
    X[k("bothinf"), c], X[k("bothinf"), c + 1] = np.inf, -np.inf        # the users' two entries there are positive
    X[k("pnan"), c] = np.float64(np.nan)
    X[k("nnan"), c] = -np.float64(np.nan)
    if X[k("e200")] @ U[0] > 0:            # finite / inf of either sign: -0.0 for the plain user, +0.0 elsewhere
        X[k("e200")] *= -1.0
    X[k("e200")] *= 1e200
    X[k("em200")] *= 1e-200
    X[k("p450")] *= 2.0 ** 450
    X[k("m450")] *= 2.0 ** -450
    X[k("m537")] *= 2.0 ** -537
    X[k("zero")] = 0.0
    v = VALUE_USERS.index
    U[v("e200")] *= 1e200
    U[v("p450")] *= 2.0 ** 450
    U[v("m450")] *= 2.0 ** -450
    U[v("em200")] *= 1e-200
    U[v("zero")] = 0.0
    U[v("zerocol"), c] = 0.0
    cand = []
    for q in range(len(VALUE_USERS)):
        lst = np.concatenate([np.arange(12), 12 + rng.permutation(N - 12)[:n - 12]]).astype(np.int32)
        cand.append(rng.permutation(lst).astype(np.int32))
    xm, um, unk = means_unknowns(rng, N, len(VALUE_USERS), d)
    return pack(X, xm, U, um, unk, cand, n, 3)


VALUE = {"value-n12": functools.partial(value_case, 12), "value-n520": functools.partial(value_case, 520)}


# ------------------------------------------------------------------ grid
GRID_NQ = [1, 3, 4, 5, 32768 + 5, 70000]
GRID_SWEEP = 32768                        # 8192 blocks x 4 waves
GRID_REPLAY = 65536                       # 1024 blocks x 64 lanes


def grid_case(nq, triple=False):
    """d = 4, lists of 0-3 rows. nq = 70000: P = 1 and every user's two
    candidates are one row under two indexes, so every user is replayed. The
    quicksort never moves a largest key behind its equal, so the replay keeps
    what the extraction already wrote; triple: P = 2 and lists (a, a', c) with
    c the best, where the replay keeps a', the later of the equal two."""
    rng = np.random.default_rng(7600 + nq + (1 if triple else 0))
    N, d = 1100, 4
    X = rows_dy(rng, N, d)
    X[(X == 0).all(axis=1)] = 1.0
    U = rows_dy(rng, nq, d)
    U[(U == 0).all(axis=1)] = 1.0
    xm = rng.integers(-32, 33, size=N).astype(np.float64) / 16.0
    um = rng.integers(-32, 33, size=nq).astype(np.float64) / 16.0
    m = rng.integers(0, d + 1, size=nq)
    up = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    ui = np.concatenate([np.sort(rng.permutation(d)[:k]) for k in m]).astype(np.int32) if nq else np.zeros(0, np.int32)
    if nq == 70000:
        X[550:] = X[:550]
        first = rng.integers(0, 550, size=nq)
        swap = rng.integers(0, 2, size=nq).astype(bool)
        pair = np.stack([first, first + 550], axis=1)
        pair[swap] = pair[swap][:, ::-1]
        P = 1
        if triple:
            # c: the user's own direction, similarity 1 (a row of the first half, so no copy of it is listed)
            lead = X[np.arange(550), (X[:550] != 0).argmax(axis=1)]
            assert len(np.unique(X[:550] / lead[:, None], axis=0)) == 550, "parallel rows: choose another seed"
            best = rng.integers(0, 550, size=nq)
            best = np.where(best == first, (best + 1) % 550, best)
            U = X[best] * 2.0
            pair = np.concatenate([pair, best[:, None]], axis=1)
            P = 2
        cp = (pair.shape[1] * np.arange(nq + 1)).astype(np.int64)
        ci = pair.ravel().astype(np.int32)
    else:
        lens = (np.arange(nq) + (3 if nq < 10 else 1)) % 4       # 0-3 rows
        if nq > GRID_SWEEP:
            lens[GRID_SWEEP:] = [1, 2, 3, 3, 2][:nq - GRID_SWEEP]      # the second sweep's users all have some
        cp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ci = rng.integers(0, N, size=int(cp[-1])).astype(np.int32)
        # no row twice in a list
        for q in np.nonzero(lens >= 2)[0]:
            while len(set(ci[cp[q]:cp[q + 1]])) < lens[q]:
                ci[cp[q]:cp[q + 1]] = rng.integers(0, N, size=int(lens[q]))
        P = 2
    for a in (xm, um, up, ui, cp, ci):
        a.setflags(write=False)
    return (X, xm, U, um, up, ui, cp, ci, P, 2)


GRID = {f"grid-nq{nq}": functools.partial(grid_case, nq) for nq in GRID_NQ}
GRID["grid-nq70000-triple"] = functools.partial(grid_case, 70000, True)


# ------------------------------------------------------------------ access
CASES = {}
for _g in (LEN, TIE, NEAR, VALUE, GRID):
    CASES.update(_g)
# families whose rows square exactly: the restatements apply
EXACT_SQUARE = [l for l in CASES if l.split("-")[0] in ("len", "tie", "grid")]


@functools.lru_cache(maxsize=None)
def case(label):
    """(X [N][d], xmean [N], U [nq][d], umean [nq], unk_ptr, unk_idx, cand_ptr,
    cand_idx, P, NTOP); built once, read-only."""
    c = CASES[label]()
    for a in c[:8]:
        a.setflags(write=False)
    return c


# ------------------------------------------------------------------ topn
TOPN_P = 5
TOPN_D = 130
TOPN_M = [0, 1, 63, 64, 65, TOPN_D]
TOPN_CNT = [0, 1, TOPN_P]
TOPN_SIMS = ["plain", "pnan", "nnan", "pinf", "ninf", "zeros", "allzero", "cancel"]
TOPN_NTOP = sorted({1} | {m for m in TOPN_M if m} | {m + 3 for m in TOPN_M})


@functools.lru_cache(maxsize=None)
def topn_case():
    """(X, xmean, umean, unk_ptr, unk_idx, nb_idx [nq][P], nb_sim, nb_cnt, meta):
    neighbour lists written by hand, one user per (cnt, kind of nb_sim row, m).
    Columns j and j + 65 of X are equal for j < 30 and columns 100..129 are all
    equal: equal predictions, ordered by the quicksort alone. Rows 30 and 31 are
    one row with one mean: under "cancel" their terms sum to zero."""
    rng = np.random.default_rng(7700)
    N, d, P = 40, TOPN_D, TOPN_P
    X = rows_dy(rng, N, d)
    X[:, 65:95] = X[:, 0:30]
    X[:, 100:130] = X[:, 100:101]
    xm = rng.integers(-32, 33, size=N).astype(np.float64) / 16.0
    X[31], xm[31] = X[30], xm[30]
    plan = [(c, k, m) for c in TOPN_CNT for k in TOPN_SIMS for m in TOPN_M]
    nq = len(plan)
    um = rng.integers(-32, 33, size=nq).astype(np.float64) / 16.0
    nb_idx = np.full((nq, P), -1, np.int32)
    nb_sim = np.zeros((nq, P))
    nb_cnt = np.zeros(nq, np.int32)
    unk = []
    pnan, nnan = np.float64(np.nan), -np.float64(np.nan)
    for q, (c, kind, m) in enumerate(plan):
        unk.append(np.arange(d, dtype=np.int32) if m == d else np.sort(rng.choice(d, size=m, replace=False)).astype(np.int32))
        nb_cnt[q] = c
        if c == 0:
            continue
        nb_idx[q, :c] = rng.choice(30, size=c, replace=False)
        s = rng.integers(-7, 8, size=c).astype(np.float64) / 8.0
        s[s == 0] = 0.5
        at = int(rng.integers(0, c))
        if kind in ("pnan", "nnan", "pinf", "ninf"):
            s[at] = {"pnan": pnan, "nnan": nnan, "pinf": np.inf, "ninf": -np.inf}[kind]
        elif kind == "zeros":
            s[at] = -0.0
            s[(at + 1) % c] = 0.0
        elif kind == "allzero":
            s[:] = 0.0
            s[::2] = -0.0                  # abs_sum == 0: every prediction is 0/0
        elif kind == "cancel" and c >= 2:
            nb_idx[q, 0], nb_idx[q, 1] = 30, 31
            s[0], s[1] = 0.5, -0.5
            s[2:] = 0.0
        nb_sim[q, :c] = s
    up, ui = csr(unk)
    out = (X, xm, um, up, ui, nb_idx, nb_sim, nb_cnt)
    for a in out:
        a.setflags(write=False)
    return out + (plan,)


# ------------------------------------------------------------------ fixtures
FIXTURES = {"recomedge_tie": "tie-P1", "recomedge_near": "near-P1", "recomedge_value": "value-n12",
            "recomedge_len": "len-P20-d24"}
INPUT_KEYS = ["x", "xmean", "u", "umean", "unk_ptr", "unk_idx", "cand_ptr", "cand_idx"]


def fixture_inputs(name):
    """The inputs of a tests/golden/recom fixture: its case, as case() gives it."""
    return case(FIXTURES[name])


def fixtures():
    return sorted(f[:-4] for f in os.listdir(DIR) if f.endswith(".npz")) if os.path.isdir(DIR) else []


def fixture(name):
    """The npz of a fixture: the inputs (INPUT_KEYS) and the reference's pc_idx,
    pc_sim, pc_cnt, top (-1 rows for users without neighbours)."""
    return np.load(os.path.join(DIR, name + ".npz"))
