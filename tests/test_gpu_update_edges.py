"""GPU: the k-means update's sum forms (csrc/update.hip) at their structural
edges, against the plain fp64 chain (km_edges.ref_sums) and the oracle, bit for
bit -- cluster boundaries placed at the chain kernel's groups, the 512-position
windows, the 64-record pair capacity and KM_LANE_MAX; one-member and empty
clusters, N = 0 / 1, K > N; the flag bits per (cluster, 64-dim block); the
sharded calls played rank by rank in one process against their numpy
restatement; km_finalize_kernel's division and movement test; reachable
carries. tests/test_update_edges_cpu.py shows on the host which branch each
input reaches; no assertion here depends on that."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import km_edges as ke
import km_shard_np as ksn
from amd import lshkm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return lshkm.Context(0)


def to_dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a)).to(ctx.dev)


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t, np.float64).view(np.uint64)


def same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} differ, first at {bad[:5].tolist()}"


# path -> (row dtype, LSHKM_KM_PATH of the test build or None for the product library, counts STAT_KM_SEQ)
PATHS = {
    "f32": (np.float32, None, True),            # fixed point; flagged chains by lanes / segments
    "f32_chain": (np.float32, "chain", False),
    "f64": (np.float64, None, False),           # binade segments
    "f64_fx": (np.float64, "fx", True),         # fixed point; flagged chains by km_chain16_kernel (no segment workspace)
    "f64_chain": (np.float64, "chain", False),
}
D_F32 = [1, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 256]    # 128, 256: km_fx2_kernel
D_OTHER = [1, 17, 64, 65, 129]


class Runner:
    """One path's calls: the product library on `ctx`, or the test build with
    its LSHKM_KM_PATH switch on `sctx`."""

    def __init__(self, path, ctx, sctx, sw, monkeypatch):
        self.dtype, self.env, self.stat = PATHS[path]
        self.mod, self.ctx = (lshkm, ctx) if self.env is None else (sw, sctx)
        self.mp = monkeypatch

    def __enter__(self):
        if self.env is not None:
            self.mp.setenv("LSHKM_KM_PATH", self.env)
        return self

    def __exit__(self, *exc):
        if self.env is not None:
            self.mp.delenv("LSHKM_KM_PATH", raising=False)

    def dev(self, a):
        return to_dev(self.ctx, a)

    def seq(self):
        return self.ctx.stat(self.mod.STAT_KM_SEQ)

    def update(self, X, A, Cd, metric="euclidean", min_dist=0.0):
        return self.mod.kmeans_update(self.ctx, X, A, Cd, metric, min_dist)

    def partial(self, X, A, K):
        return self.mod.kmeans_partial(self.ctx, X, A, K)

    def carry(self, X, A, K, cs=None, cc=None):
        return self.mod.kmeans_partial_carry(self.ctx, X, A, K, cs, cc)


@functools.lru_cache(maxsize=40)
def sweep_case(layout, fam, dtype, d):
    """Host side of one sweep case, shared by the paths of one row type."""
    sizes = ke.LAYOUTS[layout]
    a, K = ke.assignment(sizes), len(sizes)
    X = ke.family(fam, a, d, dtype)
    Cold = np.random.default_rng(5).integers(-3, 4, (K, d)).astype(np.float64)
    Co, co, cont = oracle.kmeans_update(X, a, Cold, "euclidean", 0.0)
    sums, cnt = ke.ref_sums(X, a, K)
    assert np.array_equal(cnt, co)
    return X, a, K, Cold, Co, co, cont, sums, int(ke.predicted_flagged(X, a, K).sum())


def check_update(run, X, a, K, Cold, Co, co, cont, sums, nflag, what):
    Xd, Ad, Cd = run.dev(X), run.dev(a), run.dev(Cold)
    seq0 = run.seq() if run.stat else 0
    Cn, cnt, go = run.update(Xd, Ad, Cd)
    if run.stat:
        assert run.seq() - seq0 == nflag, f"{what}: STAT_KM_SEQ"
    same(Cn, Co, f"{what}: centers")
    assert np.array_equal(cnt.cpu().numpy(), co) and go == cont, what
    s, sc = run.partial(Xd, Ad, K)
    same(s, sums, f"{what}: partial sums")
    assert np.array_equal(sc.cpu().numpy(), co), what


# ------------------------------------------------------------------ 2.1 structure sweep
@pytest.mark.parametrize("layout", sorted(ke.LAYOUTS))
@pytest.mark.parametrize("fam", ["exact", "flag_all", "flag_mix", "special"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_structure_sweep(ctx, sctx, sw, monkeypatch, path, fam, layout):
    with Runner(path, ctx, sctx, sw, monkeypatch) as run:
        for d in (D_F32 if path == "f32" else D_OTHER):
            case = sweep_case(layout, fam, run.dtype, d)
            if fam == "exact":
                assert case[-1] == 0
            check_update(run, *case, what=f"{path} {layout} {fam} d={d}")


# ------------------------------------------------------------------ 2.2 flag bits
@functools.lru_cache(maxsize=2)
def flag_block_case(d, cols, sizes):
    sizes = list(sizes)
    a, K = ke.assignment(sizes), len(sizes)
    X = ke.flag_block(a, d, list(cols))
    Cold = np.random.default_rng(5).integers(-3, 4, (K, d)).astype(np.float64)
    Co, co, cont = oracle.kmeans_update(X, a, Cold, "euclidean", 0.0)
    sums, _ = ke.ref_sums(X, a, K)
    fl = ke.predicted_flagged(X, a, K)
    assert set(np.nonzero(fl.any(axis=0))[0]) == set(cols)
    return X, a, K, Cold, Co, co, cont, sums, int(fl.sum())


@pytest.mark.parametrize("d,cols", [(130, (70,)), (2050, (1990,)), (2050, (2049,)), (2050, (1990, 2049))])
def test_flag_block_short_chains(ctx, sctx, sw, monkeypatch, d, cols):
    # K as given: a segment workspace exists and every flagged chain is short (by lanes)
    with Runner("f32", ctx, sctx, sw, monkeypatch) as run:
        case = flag_block_case(d, cols, tuple(ke.LAYOUTS["windows_a1"]))
        assert case[-1] == 5 * len(cols)                     # the clusters of two or more members
        check_update(run, *case, what=f"flag_block d={d} cols={cols}")


def test_flag_block_one_block_by_segments(ctx, sctx, sw, monkeypatch):
    # one cluster past KM_LANE_MAX at d = 130: its block 1 alone takes the
    # segment passes (flag bit 1); blocks 0 and 2 and the other clusters do not
    sizes = list(ke.LAYOUTS["windows_a1"])
    sizes[7] = 33000                                         # the cluster that started at 1300
    with Runner("f32", ctx, sctx, sw, monkeypatch) as run:
        case = flag_block_case(130, (70,), tuple(sizes))
        assert case[-1] == 5
        check_update(run, *case, what="flag_block enlarged")


def test_flag_block_without_segment_workspace(ctx, sctx, sw, monkeypatch):
    # K = 65,600 > 65,535: no segment workspace, the flagged chains go to the
    # float instantiation of the flagged km_chain16_kernel by flag bit 1 (d = 130)
    K = 65_600
    ids = [0, 7, 4097, 32768, 65535, 65536, K - 1]
    sizes = [0] * K
    for c, s in zip(ids, [s for s in ke.LAYOUTS["windows_a1"] if s]):
        sizes[c] = int(s)
    with Runner("f32", ctx, sctx, sw, monkeypatch) as run:
        case = flag_block_case(130, (70,), tuple(sizes))
        assert case[-1] == 5                                 # the clusters of 511, 511, 276, 1200 and 574 members
        check_update(run, *case, what="flag_block K=65600")


def test_certify_flag_bits(ctx):
    # lshkm_kmeans_shard_certify on hand-made exchanged values: bit min(31, j / 64)
    # of a long chain's cluster, blocks 31 and 32 sharing bit 31; short chains get
    # mask 2 and no bit
    torch = ctx.torch
    K, d = 3, 2050
    q = np.full((K, d), 1 << 30, np.int32)
    t = np.full((K, d), -(1 << 30), np.int32)
    cols = {0: [5, 2049], 1: [70, 1990, 2049], 2: [1984, 64 * 30 + 63]}
    for c, js in cols.items():
        q[c, js], t[c, js] = -40, 41
    qt = np.stack([q, -t])
    asum = np.where(q < 0, 2.0 ** 55, 0.0)
    counts = np.array([32768, 32769, 40000], np.int64)
    gathered = np.zeros((1, K, d))
    ops = lshkm.ShardSums(ctx, ctx.empty((0, d), torch.float32), None, K)
    out, start, flag, mask, nf = ops.certify(to_dev(ctx, gathered), to_dev(ctx, asum), to_dev(ctx, qt),
                                             to_dev(ctx, counts), 1, 0)
    want_mask = np.zeros((K, d), np.uint8)
    want_mask[0, cols[0]] = 2
    want_mask[1, cols[1]] = 1
    want_mask[2, cols[2]] = 1
    assert np.array_equal(mask.cpu().numpy(), want_mask) and nf == 7
    assert flag.cpu().numpy().tolist() == [0, -(1 << 31) | 2, -(1 << 31) | (1 << 30)]
    ref = ksn.NumpyShardSums(np.zeros((0, d)), np.zeros(0, np.int32), K)
    _, _, rflag, rmask, rnf = ref.certify(torch.from_numpy(gathered), torch.from_numpy(asum), torch.from_numpy(qt),
                                          torch.from_numpy(counts), 1, 0)
    assert np.array_equal(flag.cpu().numpy(), rflag.numpy()) and np.array_equal(want_mask, rmask.numpy()) and rnf == nf


# ------------------------------------------------------------------ 2.3 lane limit
@functools.lru_cache(maxsize=2)
def lanes_case(d, fam):
    a1 = ke.assignment([3, 3, 3, 1], seed=9)                 # a first shard of 10 rows
    a2 = ke.assignment(ke.LANES)
    a = np.concatenate([a1, a2])
    X = ke.family(fam, a, d, np.float32)
    return X, a, 4


@pytest.mark.parametrize("fam", ["flag_all", "flag_mix"])
@pytest.mark.parametrize("d", [3, 65])
def test_lane_limit(ctx, sctx, sw, monkeypatch, d, fam):
    # clusters of 32,767 / 32,768 / 32,769 flagged chains: lanes up to
    # KM_LANE_MAX, segments (the f32 fx + seg path) past it
    X, a, K = lanes_case(d, fam)
    X2, a2 = X[10:], a[10:]
    Cold = np.zeros((K, d))
    Co, co, cont = oracle.kmeans_update(X2, a2, Cold, "euclidean", 0.0)
    sums, _ = ke.ref_sums(X2, a2, K)
    with Runner("f32", ctx, sctx, sw, monkeypatch) as run:
        check_update(run, X2, a2, K, Cold, Co, co, cont, sums, 3 * d, what=f"lanes d={d}")


@pytest.mark.parametrize("fam", ["flag_all", "flag_mix"])
@pytest.mark.parametrize("d", [3, 65])
def test_lane_limit_with_carry(ctx, sctx, sw, monkeypatch, d, fam):
    # the carry is one more value of the chain: 32,768 members + carry = 32,769
    X, a, K = lanes_case(d, fam)
    whole, cw = ke.ref_sums(X, a, K)
    s1, _ = ke.ref_sums(X[:10], a[:10], K)
    nflag = int(ke.predicted_flagged(X[10:], a[10:], K, carry=s1).sum())
    assert nflag == (4 if fam == "flag_all" else 3) * d     # flag_mix: carry + one member passes the count form
    with Runner("f32", ctx, sctx, sw, monkeypatch) as run:
        Xd, Ad = run.dev(X), run.dev(a)
        cs, cc = run.carry(Xd[:10], Ad[:10], K)
        same(cs, s1, "first shard")
        seq0 = run.seq()
        cs, cc = run.carry(Xd[10:], Ad[10:], K, cs, cc)
        assert run.seq() - seq0 == nflag
        same(cs, whole, f"lanes with carry d={d}")
        assert np.array_equal(cc.cpu().numpy(), cw)


@pytest.mark.parametrize("K", [65_535, 65_536])
def test_long_flagged_chain_in_the_last_cluster(ctx, sctx, sw, monkeypatch, K):
    # K = 65,535: the composition grid's last y index; K = 65,536: the first K
    # without a segment workspace (km_chain16_kernel by flag bits)
    d = 2
    sizes = [0] * K
    sizes[K - 1] = 32_800
    for c in range(0, 200):
        sizes[(c * 331) % (K - 1)] += 1
    a = ke.assignment(sizes)
    X = ke.exact(a, d, np.float32)
    m = a == K - 1
    X[m] = ke.flag_all(a, d, np.float32)[m]
    Cold = np.zeros((K, d))
    Co, co, cont = oracle.kmeans_update(X, a, Cold, "euclidean", 0.0)
    sums, _ = ke.ref_sums(X, a, K)
    nflag = int(ke.predicted_flagged(X, a, K).sum())
    assert nflag == d and len(a) == 33_000
    with Runner("f32", ctx, sctx, sw, monkeypatch) as run:
        check_update(run, X, a, K, Cold, Co, co, cont, sums, nflag, what=f"K={K}")


# ------------------------------------------------------------------ 2.4 segment branches
@pytest.mark.parametrize("first", [None, 100, 512])
@pytest.mark.parametrize("name", sorted(ke.SEG_CHAINS))
@pytest.mark.parametrize("path", ["f64", "f64_chain"])
def test_segment_branches(ctx, sctx, sw, monkeypatch, path, name, first):
    # 63 / 64 / 65 / 66 records in a pair, dense pairs, failed summaries, ties: at
    # window offsets 0 and 37, d = 70 (a full and a partial 64-dim block); with a
    # carry, each chain split at 100 and at exactly 512 positions
    X, a, K, cuts = ke.seg_case(name, 70, first)
    whole, cw = ke.ref_sums(X, a, K)
    with Runner(path, ctx, sctx, sw, monkeypatch) as run:
        Xd, Ad = run.dev(X), run.dev(a)
        if first is None:
            Cold = np.zeros((K, 70))
            Co, co, cont = oracle.kmeans_update(X, a, Cold, "euclidean", 0.0)
            check_update(run, X, a, K, Cold, Co, co, cont, whole, 0, what=f"{path} {name}")
            return
        cs = cc = None
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            cs, cc = run.carry(Xd[lo:hi], Ad[lo:hi], K, cs, cc)
        same(cs, whole, f"{path} {name} split at {first}")
        assert np.array_equal(cc.cpu().numpy(), cw)


# ------------------------------------------------------------------ 2.5 sharded calls in one process
def play(ops, add, minimum, stack, clone):
    """sharding.kmeans_sums_sharded's steps for every rank of one process:
    begin on every shard; the exchange (partial sums stacked, |x| sums and
    counts summed in rank order, q / -t MIN); certify per rank; prepare on every
    rank before any chain; chain in rank order from the previous rank's out."""
    world = len(ops)
    begun = [o.begin() for o in ops]
    gathered = stack([b[0] for b in begun])
    asum, qt, counts = clone(begun[0][1]), clone(begun[0][2]), clone(begun[0][3])
    for b in begun[1:]:
        asum, qt, counts = add(asum, b[1]), minimum(qt, b[2]), add(counts, b[3])
    cert = [o.certify(gathered, asum, qt, counts, world, r) for r, o in enumerate(ops)]
    outs = [c[0] for c in cert]
    if cert[0][4]:
        for o, (_, start, flag, mask, _) in zip(ops, cert):
            o.prepare(start, flag, mask)
        carry = None
        for o, (out, _, flag, mask, _) in zip(ops, cert):
            o.chain(flag, mask, carry, out)
            carry = out
    return begun, gathered, (asum, qt, counts), cert, outs


def check_sharded(ctx, X, a, K, cuts):
    torch = ctx.torch
    world = len(cuts) - 1
    Xd, Ad = to_dev(ctx, X), to_dev(ctx, a)
    dev_ops, np_ops = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        dev_ops.append(lshkm.ShardSums(ctx, Xd[lo:hi], lshkm.clusters(ctx, Ad[lo:hi], K), K))
        np_ops.append(ksn.NumpyShardSums(X[lo:hi], a[lo:hi], K))
    tops = (lambda x, y: x + y, torch.minimum, torch.stack, lambda x: x.clone())
    db, dg, (dasum, dqt, dcounts), dcert, douts = play(dev_ops, *tops)
    with np.errstate(invalid="ignore", over="ignore"):       # inf / nan rows through the numpy restatement
        nb, ng, (nasum, nqt, ncounts), ncert, nouts = play(np_ops, *tops)
    gmask = ncert[0][3].numpy()
    bad = nqt.numpy()[0] <= -ksn.KMF_BAD // 2
    dgath = dg.cpu().numpy()
    for r in range(world):
        what = f"rank {r} of {world}"
        n = np.bincount(a[cuts[r]:cuts[r + 1]], minlength=K)
        assert np.array_equal(db[r][2].cpu().numpy(), nb[r][2].numpy()), f"{what}: qt"
        assert np.array_equal(db[r][3].cpu().numpy(), nb[r][3].numpy()) and np.array_equal(n, nb[r][3].numpy()), what
        ds, ns = db[r][0].cpu().numpy(), nb[r][0].numpy()
        assert np.array_equal(ds[gmask == 0], ns[gmask == 0]), f"{what}: partial sums where the test passes"
        da, na = db[r][1].cpu().numpy(), nb[r][1].numpy()
        lbad = nb[r][2].numpy()[0] <= -ksn.KMF_BAD // 2         # inf / nan among the values: sum |x| unused
        # both sides are n rounded adds of non-negative terms in some order: n 2^-53 relative
        tol = n[:, None] * 2.0 ** -53 * na
        err = np.abs(da - na)
        assert np.all((err <= tol) | lbad), f"{what}: asum, worst {np.max(np.where(lbad, 0.0, err / np.maximum(na, 1e-300)))}"
        dout, dstart, dflag, dmask, dnf = dcert[r]
        _, _, nflag, nmask, nnf = ncert[r]
        assert np.array_equal(dmask.cpu().numpy(), nmask.numpy()), f"{what}: mask"
        assert np.array_equal(dflag.cpu().numpy(), nflag.numpy()), f"{what}: flag"
        assert dnf == nnf, f"{what}: n_flagged"
        pre = np.zeros_like(dgath[0])
        for rr in range(r):
            pre = pre + dgath[rr]
        same(dstart, pre, f"{what}: start")
    # the global values, identical on every rank
    assert np.array_equal(dqt.cpu().numpy(), nqt.numpy()) and np.array_equal(dcounts.cpu().numpy(), ncounts.numpy())
    assert np.array_equal(ncounts.numpy(), np.bincount(a, minlength=K))
    whole, _ = ke.ref_sums(X, a, K)
    same(douts[-1], whole, "the last rank's out")
    same(nouts[-1], whole, "the numpy restatement's out")
    return gmask, bad


def dt(kind):
    return np.float32 if kind == "f32" else np.float64


@pytest.mark.parametrize("fam", ["flag_all", "flag_mix"])
@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("cut", ["one", "two_at_1024", "empty_middle_rank", "cluster_absent_on_middle_rank"])
def test_sharded_windows_flagged(ctx, kind, cut, fam):
    sizes = np.asarray(ke.LAYOUTS["windows_a1"])
    K, d = len(sizes), 70
    if cut == "one":
        per = [sizes]
    elif cut == "two_at_1024":                               # the cut at a multiple of 512
        first = ke.split_sizes(sizes, [1 / 3, 2 / 3])[0]
        first[0] += 1024 - first.sum()
        per = [first, sizes - first]
    elif cut == "empty_middle_rank":
        first = ke.split_sizes(sizes, [0.4, 0.6])[0]
        per = [first, np.zeros_like(sizes), sizes - first]
    else:
        per = ke.split_sizes(sizes, [0.3, 0.3, 0.4])
        per[2][7] += per[1][7]                               # the cluster [1300, 2500): none on the middle rank
        per[1][7] = 0
    a, cuts = ke.sharded_assignment(per)
    if cut == "two_at_1024":
        assert cuts[1] == 1024
    X = ke.family(fam, a, d, dt(kind))
    gmask, _ = check_sharded(ctx, X, a, K, cuts)
    assert np.array_equal(gmask != 0, (sizes >= (2 if fam == "flag_all" else 3))[:, None] & np.ones((1, d), bool))
    assert set(np.unique(gmask)) == {0, 2}


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharded_singletons_special(ctx, kind, world):
    sizes = np.asarray(ke.LAYOUTS["singletons"])
    idx = np.arange(len(sizes))
    big = int(np.argmax(sizes))
    share = ke.split_sizes([600], [1.0 / world] * world)
    per = []
    for r in range(world):                                   # one-member clusters dealt round the ranks
        per.append(np.where(sizes == 1, (idx % world == r).astype(np.int64), 0))
        per[r][big] = share[r][0]
    assert np.array_equal(sum(per), sizes)
    a, cuts = ke.sharded_assignment(per)
    X = ke.special(a, 17, dt(kind))
    check_sharded(ctx, X, a, len(sizes), cuts)


@pytest.mark.parametrize("fam", ["flag_all", "flag_mix"])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_sharded_lanes_by_global_count(ctx, kind, fam):
    # the global count decides: 32,769 = 20,000 + 12,769 is mask 1 (segments) on
    # both ranks; 32,768 = 16,384 + 16,384 and 32,767 are mask 2 (lanes)
    first = np.array([10_000, 16_384, 20_000, 0])
    per = [first, np.asarray(ke.LANES) - first]
    a, cuts = ke.sharded_assignment(per)
    X = ke.family(fam, a, 3, dt(kind))
    gmask, _ = check_sharded(ctx, X, a, 4, cuts)
    assert gmask.tolist() == [[2] * 3, [2] * 3, [1] * 3, [0] * 3]


def test_sharded_segments_at_flag_bit_31(ctx):
    # d = 2050 with a reported global count past KM_LANE_MAX (as if further ranks
    # held the rest of each cluster): the flagged chains of columns 70, 1990 and
    # 2049 take the segment passes by flag bits 1 and 31, the latter shared by
    # blocks 31 and 32; the chains over this rank's rows equal the reference
    torch = ctx.torch
    sizes = ke.LAYOUTS["windows_b1"]
    a, K, d = ke.assignment(sizes), len(sizes), 2050
    X = ke.flag_block(a, d, [70, 1990, 2049])
    ops = lshkm.ShardSums(ctx, to_dev(ctx, X), lshkm.clusters(ctx, to_dev(ctx, a), K), K)
    sums, asum, qt, counts = ops.begin()
    out, start, flag, mask, nf = ops.certify(sums.reshape((1, K, d)), asum, qt, counts + 40_000, 1, 0)
    live = np.asarray(sizes) >= 1
    m = mask.cpu().numpy()
    assert np.all(m[live][:, [70, 1990, 2049]] == 1) and m.sum() == 3 * live.sum() and nf == 3 * live.sum()
    assert flag.cpu().numpy().tolist() == [(-(1 << 31) | 2) if s else 0 for s in sizes]
    ops.prepare(start, flag, mask)
    ops.chain(flag, mask, None, out)
    whole, _ = ke.ref_sums(X, a, K)
    same(out, whole, "segments at d = 2050")


def test_shard_prepare_rejects_bad_arguments(ctx):
    torch = ctx.torch
    N, d, K = 600, 2, 4
    a = ke.assignment([100, 200, 0, 300])
    X = to_dev(ctx, ke.exact(a, d, np.float32))
    crow, rows = lshkm.clusters(ctx, to_dev(ctx, a), K)
    nb = C.c_int64()
    lshkm._ck(lshkm.lib().lshkm_kmeans_shard_ws_bytes(N, K, d, C.byref(nb)))
    ws = ctx.torch.full((nb.value,), 0x5A, dtype=torch.uint8, device=ctx.dev)
    start = ctx.torch.zeros((K, d), dtype=torch.float64, device=ctx.dev)
    flag = ctx.torch.zeros((K,), dtype=torch.int32, device=ctx.dev)
    mask = ctx.torch.zeros((K, d), dtype=torch.uint8, device=ctx.dev)
    p = lshkm._t_ptr
    rc = lshkm.lib().lshkm_kmeans_shard_prepare(ctx.h, p(X), N, d, p(crow), p(rows), K, p(start), p(flag), p(mask),
                                                p(ws), nb.value - 1)
    assert rc != 0
    K2 = 65_536
    crow2 = ctx.torch.full((K2 + 1,), N, dtype=torch.int64, device=ctx.dev)
    crow2[0] = 0
    start2 = ctx.torch.zeros((K2, d), dtype=torch.float64, device=ctx.dev)
    flag2 = ctx.torch.zeros((K2,), dtype=torch.int32, device=ctx.dev)
    mask2 = ctx.torch.zeros((K2, d), dtype=torch.uint8, device=ctx.dev)
    rc = lshkm.lib().lshkm_kmeans_shard_prepare(ctx.h, p(X), N, d, p(crow2), p(rows), K2, p(start2), p(flag2),
                                                p(mask2), p(ws), nb.value)
    assert rc != 0
    ctx.sync()
    assert bool((ws == 0x5A).all())                          # nothing was launched: the workspace is untouched
    lshkm._ck(lshkm.lib().lshkm_kmeans_shard_prepare(ctx.h, p(X), N, d, p(crow), p(rows), K, p(start), p(flag), p(mask),
                                                     p(ws), nb.value))
    ctx.sync()
    assert not bool((ws == 0x5A).all())                      # the accepted call does write it


# ------------------------------------------------------------------ 2.6 finalize
@pytest.mark.parametrize("d", [1, 64, 65, 129])
def test_finalize_strictness_and_division(ctx, d):
    K = 5
    rng = np.random.default_rng(d)
    Cold = rng.integers(-50, 51, (K, d)).astype(np.float64)
    counts = np.array([3, 7, 0, 1, 11], np.int64)
    div = np.where(counts == 0, 1, counts)[:, None].astype(np.float64)
    hi = 64 if d > 64 else d - 1                             # the second moved dim (beyond lane 63 when d > 64)
    for moved in (0, 1, 3, 4):
        delta = np.zeros((K, d))
        if d == 1:
            delta[moved, 0], dist = 3.0, 3.0
        else:
            delta[moved, 0], delta[moved, hi], dist = 3.0, -4.0, 5.0
        sums = (Cold + delta) * div                          # exact integers; the empty cluster's sum is Cold itself
        want = np.where(counts[:, None] != 0, sums / div, sums)
        assert np.array_equal(want, Cold + delta)
        for min_dist, go in ((dist, False), (np.nextafter(dist, 0.0), True), (np.nextafter(dist, 9.0), False)):
            Cn, cont = lshkm.kmeans_finalize(ctx, to_dev(ctx, sums), to_dev(ctx, counts), to_dev(ctx, Cold), "euclidean",
                                             min_dist)
            same(Cn, want, f"d={d} moved={moved}")
            assert cont == go, f"d={d} moved={moved} min_dist={min_dist!r}: dist > min_dist is strict"
    # a count of 0 leaves the sum undivided, whatever it holds; other counts divide every dim
    sums = rng.standard_normal((K, d)) * 1000
    want = np.where(counts[:, None] != 0, sums / div, sums)
    Cn, cont = lshkm.kmeans_finalize(ctx, to_dev(ctx, sums), to_dev(ctx, counts), to_dev(ctx, Cold), "euclidean", 0.0)
    same(Cn, want, f"d={d} division")
    assert cont


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("d", [17, 129])
def test_finalize_matches_oracle(ctx, metric, d):
    sizes = ke.LAYOUTS["groups"]
    a, K = ke.assignment(sizes), len(sizes)
    X = ke.exact(a, d, np.float64)
    sums, cnt = ke.ref_sums(X, a, K)
    Cold = np.random.default_rng(8).standard_normal((K, d))
    for min_dist in (0.0, 1e-3, 0.5, 1e9):
        Co, co, cont = oracle.kmeans_update(X, a, Cold, metric, min_dist)
        Cn, go = lshkm.kmeans_finalize(ctx, to_dev(ctx, sums), to_dev(ctx, cnt), to_dev(ctx, Cold), metric, min_dist)
        same(Cn, Co, f"{metric} d={d}")
        assert go == cont, f"{metric} d={d} min_dist={min_dist}"


# ------------------------------------------------------------------ 2.7 reachable carries
@pytest.mark.parametrize("path", sorted(PATHS))
def test_reachable_carries(ctx, sctx, sw, monkeypatch, path):
    # carries a previous call really produces: +0.0 into a cluster that is empty
    # on both shards, inf and nan from the first shard's values, and a finite
    # carry through clusters with no member on the second shard
    K, d = 8, 70
    first = np.array([300, 40, 0, 513, 64, 5, 0, 1])
    second = np.array([200, 0, 0, 700, 0, 65, 0, 0])          # clusters 1, 4, 7: carry passes through; 2, 6: empty
    a, cuts = ke.sharded_assignment([first, second])
    with Runner(path, ctx, sctx, sw, monkeypatch) as run:
        X = ke.exact(a, d, run.dtype)
        r1 = np.nonzero(a[:cuts[1]] == 1)[0]
        r0 = np.nonzero(a[:cuts[1]] == 0)[0]
        X[r1[3], 5], X[r1[7], 9] = np.inf, np.nan             # inf / nan carries that pass through unchanged
        X[r0[2], 5], X[r0[4], 9] = np.inf, np.nan             # ... and into more members
        X[r0[6], 11] = 3.0e30                                 # a carry that flags the fixed point's chain
        whole, cw = ke.ref_sums(X, a, K)
        s1, c1 = ke.ref_sums(X[:cuts[1]], a[:cuts[1]], K)
        assert np.isinf(s1[1, 5]) and np.isnan(s1[1, 9]) and not np.signbit(s1[2]).any()
        Xd, Ad = run.dev(X), run.dev(a)
        cs, cc = run.carry(Xd[:cuts[1]], Ad[:cuts[1]], K)
        same(cs, s1, f"{path}: first shard")
        cs, cc = run.carry(Xd[cuts[1]:], Ad[cuts[1]:], K, cs, cc)
        same(cs, whole, f"{path}: second shard")
        assert np.array_equal(cc.cpu().numpy(), cw)
        for c in (1, 4, 7, 2, 6):
            assert np.array_equal(bits(cs)[c], s1[c].view(np.uint64))
