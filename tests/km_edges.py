"""Inputs for the k-means update's structural edges (csrc/update.hip), and the
plain reference they are checked against. CPU only: numpy, no GPU import.

A *layout* is a list of cluster sizes; crow = its running total. assignment()
turns it into a per-row cluster id by a fixed-seed shuffle of the row
positions, so the cluster-sorted row list is never the identity while member
order stays row order. A *value family* fills the rows; each has a stated
property (which chains km_cert rejects, how many segment records a pair holds)
that tests/test_update_edges_cpu.py verifies on the host. The GPU assertions
(tests/test_gpu_update_edges.py) never depend on the property: it only shows
that the branch is reached.

The reference is the reference program's own operation restated plainly: for
each (c, j) one sequential fp64 chain over the members of c in row order, from
the carry or +0.0 (ref_sums). Centers, counts and `cont` come from
oracle.kmeans_update."""
import numpy as np

import km_shard_np as ksn

KS_W = 512              # window / chunk (KS_W, KMF_CH)
KS_R = 64               # records per pair
KM_LANE_MAX = 32768


# ------------------------------------------------------------------ layouts
def crow_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def assignment(sizes, seed=7):
    """Per-row cluster ids of a layout: cluster c owns sizes[c] rows, at
    shuffled row positions."""
    sizes = np.asarray(sizes, np.int64)
    a = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return a[np.random.default_rng(seed).permutation(len(a))]


def sharded_assignment(per_rank_sizes, seed=7):
    """Rows of consecutive shards: shard r holds per_rank_sizes[r][c] members
    of cluster c, shuffled within the shard. Returns (assign, cuts): shard r is
    rows cuts[r]:cuts[r + 1]."""
    parts, cuts = [], [0]
    for r, sizes in enumerate(per_rank_sizes):
        parts.append(assignment(sizes, seed + 101 * r))
        cuts.append(cuts[-1] + len(parts[-1]))
    return np.concatenate(parts).astype(np.int32), cuts


def split_sizes(sizes, fractions):
    """Cut every cluster of a layout over len(fractions) shards in proportion
    (the last shard takes the remainder)."""
    sizes = np.asarray(sizes, np.int64)
    out, left = [], sizes.copy()
    for f in fractions[:-1]:
        take = np.minimum(left, (sizes * f).astype(np.int64))
        out.append(take)
        left = left - take
    out.append(left)
    return out


# chain groups of 64 (KM16_G), the 4-group unroll and the 3-group look-ahead
# (KM16_Q): ng = 1..9, partial last groups of 1-3 rows, every residue of ng mod
# 4 (447..449 added for ng = 7, which the other sizes skip). 5,775 rows.
GROUPS = [0, 1, 2, 3, 4, 5, 0, 63, 64, 65, 0, 0, 127, 128, 129, 191, 192, 193, 0, 255, 256, 257, 319, 320, 321, 447,
          448, 449, 511, 512, 513, 0]


def windows(shape, extra):
    """Boundaries at absolute positions of the 512-position windows. shape "a":
    crow holds 511, 512 and 513; shape "b": one cluster is exactly [512, 1024).
    Both: two empty clusters whose crow is the window edge 1024, a cluster
    [1300, 2500) that starts mid-window and spans three windows, and the last
    cluster ending exactly at M = 3072 + extra (extra 0 or 1)."""
    bounds = {"a": [0, 511, 512, 513, 1024, 1024, 1024, 1300, 2500, 3072 + extra],
              "b": [0, 512, 1024, 1024, 1024, 1300, 2500, 3072 + extra]}[shape]
    return list(np.diff(bounds))


def singletons():
    """1,300 one-member clusters, one of 600, 200 more of one member; every 7th
    id is empty. Hundreds of pairs in one window (pair index w + c), a flush /
    open / close at every step, one-member chains."""
    sizes = []
    for s in [1] * 1300 + [600] + [1] * 200:
        if len(sizes) % 7 == 6:
            sizes.append(0)
        sizes.append(s)
    return sizes


def scattered(K, members):
    sizes = [0] * K
    for c in members:
        sizes[c] += 1
    return sizes


LAYOUTS = {
    "groups": GROUPS,
    "windows_a0": windows("a", 0),
    "windows_a1": windows("a", 1),
    "windows_b0": windows("b", 0),
    "windows_b1": windows("b", 1),
    "singletons": singletons(),
    "n0_k3": [0, 0, 0],
    "n1_first": [1, 0, 0, 0, 0],
    "n1_last": [0, 0, 0, 0, 1],
    "k40_n7": scattered(40, [0, 5, 5, 13, 21, 38, 39]),
    "empty_ends": [0, 0, 0, 16, 17, 15, 0, 0, 0],
}
LANES = [32767, 32768, 32769, 1]          # KM_LANE_MAX; run at d in {3, 65} only


# ------------------------------------------------------------------ values
def member_rank(a):
    """Position of each row among its cluster's members (row order)."""
    a = np.asarray(a)
    order = np.argsort(a, kind="stable")
    sa = a[order]
    first = np.concatenate([[0], np.nonzero(np.diff(sa))[0] + 1]) if len(a) else np.zeros(0, np.int64)
    start = np.zeros(len(a), np.int64)
    if len(a):
        start[first] = first
        start = np.maximum.accumulate(start)
    rank = np.empty(len(a), np.int64)
    rank[order] = np.arange(len(a)) - start
    return rank


def col_scale(d):
    """Per-column power-of-two scale and sign: columns differ, bit structure does not."""
    j = np.arange(d)
    return np.ldexp(np.where(j % 2 == 0, 1.0, -1.0), (j % 5) - 2)


def exact(a, d, dtype, seed=3):
    """Integers in [-1000, 1000] times 2^-3: every chain passes km_cert."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-1000, 1001, (len(a), d)) * 0.125).astype(dtype)


def flag_all(a, d, dtype):
    """2^40 and 3 * 2^-40 alternating along each cluster's members (times a
    per-column power of two and sign): every chain of >= 2 members holds both,
    so lc + t - q >= 82 and sum |x| >= 2^27 times the |x| bound; one-member
    chains pass."""
    big = (member_rank(a) % 2 == 0)[:, None]
    X = np.where(big, 2.0 ** 40, 3.0 * 2.0 ** -40) * col_scale(d)[None, :]
    return X.astype(dtype)


def flag_mix(a, d, dtype, seed=3):
    """Odd 24-bit integers times 2^20, 1 and 2^-20 by member position mod 3:
    every chain of >= 3 members fails both bounds of km_cert (t - q >= 64), and
    unlike flag_all its partial sums round at almost every step, so the result
    depends on the order of the adds."""
    rng = np.random.default_rng(seed)
    m = (rng.integers(1 << 22, 1 << 23, (len(a), d)) * 2 + 1) * rng.choice([-1.0, 1.0], (len(a), d))
    e = (20 - 20 * (member_rank(a) % 3)).astype(np.int32)[:, None]
    return np.ldexp(m, e).astype(dtype)


def flag_block(a, d, cols, seed=3):
    """f32 `exact` with flag_all's values in the columns `cols` only."""
    X = exact(a, d, np.float32, seed)
    F = flag_all(a, d, np.float32)
    for j in cols:
        X[:, j] = F[:, j]
    return X


def special(a, d, dtype, seed=3):
    """`exact` plus one inf, one nan, one -0.0, one denormal and one huge value
    (3e30 / 1.5e308), in distinct rows and (for d >= 5) distinct columns."""
    X = exact(a, d, dtype, seed)
    N = len(a)
    f32 = np.dtype(dtype) == np.float32
    vals = [np.inf, np.nan, -0.0, 1e-42 if f32 else 1e-310, 3.0e30 if f32 else 1.5e308]
    for k, v in enumerate(vals):
        if N:
            X[(k * 7919 + N // 3) % N, (2 * k + 1) % d] = v
    return X


FAMILIES = {"exact": exact, "flag_all": flag_all, "flag_mix": flag_mix, "special": special}


def family(name, a, d, dtype):
    return FAMILIES[name](a, d, dtype)


# ------------------------------------------------------------------ f64 segment chains
def chain_records(F, n=700):
    """Start 1.25, steps of 2^-20, and F flips of -1.0 / +1.0 (every third
    position): the partial sums leave and re-enter [1, 2) F times, F + 1 records
    in the
    chain's first window (the rest of the chain is one more record)."""
    x = np.full(n, 2.0 ** -20)
    x[0] = 1.25
    for f in range(F):
        x[3 + 3 * f] = -1.0 if f % 2 == 0 else 1.0
    return x


def chain_dense(n=1100):
    """1.5, then -1.0 / +1.0 alternating: the partial sum changes binade at every step."""
    x = np.where(np.arange(n) % 2 == 1, -1.0, 1.0)
    x[0] = 1.5
    return x


def chain_fallback():
    """2^60, 1,023 x 1.0, -2^60, 1,023 x 1.0: the pair starts predicted from
    pair sums disagree with the true chain after the cancellation."""
    x = np.ones(2048)
    x[0], x[1024] = 2.0 ** 60, -(2.0 ** 60)
    return x


def chain_ties(n=1500, seed=23):
    """The dyadic values of test_gpu_update's "ties" kind: with the carry-free
    start 2^44 the grid is coarse and many steps are exact ties."""
    rng = np.random.default_rng(seed)
    x = np.ldexp(np.round(rng.standard_normal(n) * 64), -7)
    x[0] += 2.0 ** 44
    return x


SEG_CHAINS = {"records62": lambda: chain_records(62), "records63": lambda: chain_records(63),
              "records64": lambda: chain_records(64), "records65": lambda: chain_records(65),
              "dense": chain_dense, "fallback": chain_fallback, "ties": chain_ties}
SEG_OFFSET = 37


def seg_layout(n):
    """[chain at window offset 0 | filler | chain at window offset 37 | filler]."""
    fill = (SEG_OFFSET - n) % KS_W
    return [n, fill if fill else KS_W, n, 11]


def seg_case(name, d=70, first=None):
    """Rows whose clusters 0 and 2 hold the crafted chain in every column (times
    a per-column power of two and sign), at window offsets 0 and 37 of the
    cluster-sorted list; clusters 1 and 3 hold `exact` filler. first: members of
    every cluster in a first shard (None: one shard). -> (X, a, K, cuts)."""
    x = SEG_CHAINS[name]()
    sizes = seg_layout(len(x))
    assert crow_of(sizes)[2] % KS_W == SEG_OFFSET
    if first is None:
        a, cuts = assignment(sizes), [0, int(sum(sizes))]
    else:
        f = np.minimum(sizes, [first, sizes[1] // 2, first, 3])
        a, cuts = sharded_assignment([f, np.asarray(sizes) - f])
    X = exact(a, d, np.float64)
    rank = member_rank(a)
    j = np.arange(d)
    scale = np.ldexp(np.where(j % 2 == 0, 1.0, -1.0), (j % 7) - 3)
    for c in (0, 2):
        m = a == c
        X[m] = x[rank[m]][:, None] * scale[None, :]
    return X, a, len(sizes), cuts


# ------------------------------------------------------------------ reference
def ref_sums(X, a, K, carry=None):
    """(sums [K][d], counts [K]): per (c, j) the sequential fp64 chain over the
    members of c in row order, from carry[c][j] or +0.0."""
    X64 = np.asarray(X).astype(np.float64)
    d = X64.shape[1]
    sums = np.zeros((K, d)) if carry is None else np.array(carry, np.float64)
    order = np.argsort(a, kind="stable")
    cr = crow_of(np.bincount(a, minlength=K))
    with np.errstate(all="ignore"):
        for c in np.nonzero(np.diff(cr))[0]:
            rows = order[cr[c]:cr[c + 1]]
            sums[c] = np.cumsum(np.concatenate([sums[c][None, :], X64[rows]]), axis=0)[-1]    # strictly in order
    return sums, np.diff(cr).astype(np.int64)


def cert_inputs(X, a, K, carry=None):
    """(q, t, cnt, asum, bad) of every (c, j) as km_fx_finalize_kernel forms
    them: the members' values, plus the carry as one more value of the chain."""
    X64 = np.asarray(X).astype(np.float64)
    d = X64.shape[1]
    if carry is not None:
        X64 = np.concatenate([X64, np.asarray(carry, np.float64)])
        a = np.concatenate([a, np.arange(K, dtype=np.int32)])
    qv, tv = ksn.bit_positions(np.where(np.isfinite(X64), X64, 0.0))
    fin = np.isfinite(X64)
    nz = (X64 != 0) & fin
    q = np.full((K, d), 1 << 30, np.int64)
    t = np.full((K, d), -(1 << 30), np.int64)
    asum = np.zeros((K, d))
    bad = np.zeros((K, d), bool)
    order = np.argsort(a, kind="stable")
    cnt = np.bincount(a, minlength=K).astype(np.int64)
    cr = crow_of(cnt)
    for c in np.nonzero(cnt)[0]:
        r = order[cr[c]:cr[c + 1]]
        q[c] = np.where(nz[r], qv[r], 1 << 30).min(axis=0)
        t[c] = np.where(nz[r], tv[r], -(1 << 30)).max(axis=0)
        asum[c] = np.where(fin[r], np.abs(X64[r]), 0.0).sum(axis=0)
        bad[c] = (~fin[r]).any(axis=0)
    q[bad] = -ksn.KMF_BAD
    return q, t, cnt, asum, bad


def predicted_flagged(X, a, K, carry=None):
    """[K][d] bool: the chains km_cert rejects on these values (STAT_KM_SEQ
    counts them)."""
    q, t, cnt, asum, _ = cert_inputs(X, a, K, carry)
    return ~ksn.km_cert(q, t, cnt, asum)


def cert_margin_ok(X, a, K, carry=None):
    """True when every chain's verdict sits at least a factor 2 from both bounds
    of km_cert (one unit of lc + t - q; a factor 2 of sum |x|), so the device's
    any-order sum |x| cannot flip it."""
    q, t, cnt, asum, bad = cert_inputs(X, a, K, carry)
    live = ~bad & (q <= t) & (cnt > 1)[:, None]         # a one-term sum |x| is exact
    lc = np.ceil(np.log2(np.maximum(cnt, 1))).astype(np.int64)[:, None] * np.ones_like(q)
    count_pass = (lc + t - q <= 53) & (lc + t <= 1023)
    count_far = ((lc + t - q <= 52) & (lc + t <= 1022)) | ((lc + t - q >= 55) | (lc + t >= 1025))
    with np.errstate(over="ignore"):
        lim = np.ldexp(1.0, np.minimum(53 + q, 1024).astype(np.int32))
        abs_pass_far = asum * 2.0 < lim
        abs_fail_far = asum > lim * 2.0
    # passing chains: the count form alone decides (no use of sum |x|), or the
    # |x| form passes with a factor 2 to spare; failing chains fail both far off
    ok = np.where(count_pass, True, abs_pass_far | (abs_fail_far & count_far))
    return bool(np.all(ok | ~live))
