"""CPU checks of tests/km_edges.py: every layout's boundaries by value, every
value family's stated property (on the host model of the segmented chain,
tests/kmseg_probe.cpp, and on km_cert restated in tests/km_shard_np.py), and
the plain numpy reference against the oracle. These are what make the GPU
tests of tests/test_gpu_update_edges.py reach the branches they name."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import km_edges as ke
import km_shard_np as ksn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kmseg_probe")
    exe = tmp / "kmseg_probe"
    subprocess.run(["g++", "-O1", "-std=c++14", "-o", str(exe), os.path.join(ROOT, "tests", "kmseg_probe.cpp")],
                   check=True)

    def run(x, start=0.0, offset=0):
        path = tmp / "chain.bin"
        np.concatenate([[start, float(offset)], x]).astype("<f8").tofile(path)
        out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        print(out.stdout.strip())
        f = dict(kv.split("=") for kv in out.stdout.split())
        return {"pairs": int(f["pairs"]), "counts": [int(c) for c in f["counts"].split(",")], "fails": int(f["fails"]),
                "dense": int(f["dense"]), "equal": int(f["equal"])}
    return run


# ------------------------------------------------------------------ layouts
def test_groups_layout():
    sizes = ke.LAYOUTS["groups"]
    want = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 447, 448, 449, 511,
            512, 513]
    assert sorted(set(sizes)) == want
    assert sizes.count(0) >= 4 and sizes[0] == 0 and sizes[-1] == 0
    ng = {(s + 63) // 64 for s in sizes}
    assert ng == set(range(10))                                      # 0 and 1..9 groups of 64
    assert {s % 64 for s in sizes if s > 5} >= {63, 0, 1}            # partial last groups of 63, 64 and 1 positions
    assert {s % 4 for s in sizes} == {0, 1, 2, 3}                    # last 4-row step of 1..4 rows
    assert {((s + 63) // 64) % 4 for s in sizes if s} == {0, 1, 2, 3}    # the unroll ends at each residue
    assert sum(sizes) == 5775


@pytest.mark.parametrize("shape,extra", [("a", 0), ("a", 1), ("b", 0), ("b", 1)])
def test_windows_layout(shape, extra):
    sizes = ke.LAYOUTS[f"windows_{shape}{extra}"]
    crow = ke.crow_of(sizes)
    M = int(crow[-1])
    assert M == 3072 + extra and (M % 512 == extra)
    pairs = list(zip(crow[:-1], crow[1:]))
    if shape == "a":
        assert {511, 512, 513} <= set(crow.tolist())
    else:
        assert (512, 1024) in pairs and (0, 512) in pairs            # clusters that are exactly one window
    assert pairs.count((1024, 1024)) == 2                            # two empty clusters at a window edge
    assert (1300, 2500) in pairs                                     # starts mid-window, spans three windows
    assert 1300 % 512 != 0 and 2499 // 512 - 1300 // 512 == 2
    assert pairs[-1][1] == M and pairs[-1][0] < M                    # the last cluster ends exactly at M


def test_singletons_layout():
    sizes = ke.LAYOUTS["singletons"]
    assert sorted(s for s in sizes if s) == [1] * 1500 + [600]
    assert all(sizes[c] == 0 for c in range(6, len(sizes), 7))       # every 7th id is empty
    assert all(sizes[c] != 0 for c in range(len(sizes)) if c % 7 != 6)
    big = sizes.index(600)
    assert sum(1 for s in sizes[:big] if s == 1) == 1300 and sum(1 for s in sizes[big + 1:] if s == 1) == 200
    crow = ke.crow_of(sizes)
    assert crow[big] == 1300 and crow[-1] == 2100
    # windows 0 and 1 hold only one-member clusters: 512 pairs each
    assert np.searchsorted(crow, 512, side="left") - np.searchsorted(crow, 0, side="left") >= 512


def test_degenerate_layouts():
    L = ke.LAYOUTS
    assert L["n0_k3"] == [0, 0, 0]
    assert L["n1_first"] == [1, 0, 0, 0, 0] and L["n1_last"] == [0, 0, 0, 0, 1]
    assert len(L["k40_n7"]) == 40 and sum(L["k40_n7"]) == 7
    assert L["empty_ends"] == [0, 0, 0, 16, 17, 15, 0, 0, 0]
    assert ke.LANES == [32767, 32768, 32769, 1] and sum(ke.LANES) == 98305
    assert ke.KM_LANE_MAX == 32768


@pytest.mark.parametrize("name", sorted(ke.LAYOUTS))
def test_assignment_is_a_shuffle_of_the_layout(name):
    sizes = ke.LAYOUTS[name]
    a = ke.assignment(sizes)
    assert np.array_equal(np.bincount(a, minlength=len(sizes)), sizes)
    if len(a) > 8:
        rows = np.argsort(a, kind="stable")
        assert not np.array_equal(rows, np.arange(len(a)))            # the sorted row list is not the identity
    rank = ke.member_rank(a)
    for c in np.unique(a)[:50]:
        assert np.array_equal(rank[a == c], np.arange(sizes[c]))


def test_sharded_assignment_and_seg_layouts():
    per = ke.split_sizes(ke.LANES, [0.61, 0.39])
    a, cuts = ke.sharded_assignment(per)
    assert np.array_equal(np.bincount(a, minlength=4), ke.LANES) and cuts[-1] == 98305
    assert np.array_equal(np.bincount(a[:cuts[1]], minlength=4), per[0])
    for name in ke.SEG_CHAINS:
        for first in (None, 100, 512):
            X, a, K, cuts = ke.seg_case(name, d=6, first=first)
            x = ke.SEG_CHAINS[name]()
            crow = ke.crow_of(np.bincount(a, minlength=K))
            assert crow[0] % 512 == 0 and crow[2] % 512 == ke.SEG_OFFSET
            for c in (0, 2):
                assert np.array_equal(X[a == c][:, 0], x * 2.0 ** -3) and np.array_equal(X[a == c][:, 1], -x * 2.0 ** -2)
                if first is not None:
                    assert np.count_nonzero(a[:cuts[1]] == c) == first


# ------------------------------------------------------------------ segment families
@pytest.mark.parametrize("offset", [0, ke.SEG_OFFSET])
def test_records_family_fills_a_pair_to_63_64_65_66(probe, offset):
    got = {F: probe(ke.chain_records(F), offset=offset) for F in (62, 63, 64, 65)}
    assert [got[F]["counts"] for F in (62, 63, 64, 65)] == [[63, 1], [64, 1], [65, 1], [66, 1]]
    assert [got[F]["dense"] for F in (62, 63, 64, 65)] == [0, 0, 1, 1]       # 64 records: lane per record; 65: dense
    assert all(g["equal"] == 1 for g in got.values())
    # a power-of-two scale and a sign (the columns of seg_case) leave the structure alone
    assert probe(-0.125 * ke.chain_records(63), offset=offset)["counts"] == [64, 1]


@pytest.mark.parametrize("offset", [0, ke.SEG_OFFSET])
def test_fallback_family_fails_summaries(probe, offset):
    g = probe(ke.chain_fallback(), offset=offset)
    assert g["fails"] >= 1 and g["dense"] == 0 and g["equal"] == 1
    assert g["fails"] == (3 if offset == 0 else 6)                   # as the issue records them
    g = probe(-8.0 * ke.chain_fallback(), offset=offset)
    assert g["fails"] >= 1 and g["dense"] == 0 and g["equal"] == 1


@pytest.mark.parametrize("offset", [0, ke.SEG_OFFSET])
def test_dense_family_has_only_dense_pairs(probe, offset):
    g = probe(ke.chain_dense(), offset=offset)
    assert g["pairs"] == 3 and g["dense"] == g["pairs"] and all(c > ke.KS_R for c in g["counts"]) and g["equal"] == 1


@pytest.mark.parametrize("offset", [0, ke.SEG_OFFSET])
def test_ties_family_on_the_host_model(probe, offset):
    g = probe(ke.chain_ties(), offset=offset)
    assert g["equal"] == 1 and g["dense"] == 0 and max(g["counts"]) > 8      # the ties break segments


# ------------------------------------------------------------------ fixed-point families
ALL_LAYOUTS = sorted(ke.LAYOUTS) + ["lanes"]


def layout(name):
    return ke.LANES if name == "lanes" else ke.LAYOUTS[name]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ALL_LAYOUTS)
def test_flag_all_flags_every_chain_of_two_or_more(name, dtype):
    sizes = layout(name)
    a, K, d = ke.assignment(sizes), len(sizes), 3 if name == "lanes" else 17
    X = ke.flag_all(a, d, dtype)
    want = (np.asarray(sizes) >= 2)[:, None] & np.ones((1, d), bool)
    assert np.array_equal(ke.predicted_flagged(X, a, K), want)
    assert ke.cert_margin_ok(X, a, K)
    # the stated margins: lc + t - q >= 82, sum |x| >= 2^27 times the |x| limit
    q, t, cnt, asum, bad = ke.cert_inputs(X, a, K)
    big = cnt >= 2
    lc = np.ceil(np.log2(np.maximum(cnt, 1))).astype(np.int64)[:, None]
    assert not bad.any() and np.all((lc + t - q)[big] >= 82)
    assert np.all(asum[big] >= 2.0 ** 27 * np.ldexp(1.0, (53 + q[big]).astype(np.int32)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ALL_LAYOUTS)
def test_flag_mix_flags_chains_of_three_and_depends_on_order(name, dtype):
    sizes = layout(name)
    a, K, d = ke.assignment(sizes), len(sizes), 3 if name == "lanes" else 17
    X = ke.flag_mix(a, d, dtype)
    assert np.array_equal(X.astype(np.float64).astype(dtype), X)
    want = (np.asarray(sizes) >= 3)[:, None] & np.ones((1, d), bool)
    assert np.array_equal(ke.predicted_flagged(X, a, K), want)
    assert ke.cert_margin_ok(X, a, K)
    # the reversed chain differs wherever a chain is long enough to round
    sums, _ = ke.ref_sums(X, a, K)
    back, _ = ke.ref_sums(X[::-1], a[::-1], K)
    long = np.asarray(sizes) >= 63
    if long.any():
        assert np.mean(sums[long] != back[long]) > 0.5


def test_flag_all_at_every_chain_length_to_32769():
    # km_cert itself at n = 2 .. 32,769 members of the alternating values
    n = np.arange(2, 32770)
    q = np.full((len(n), 1), -40, np.int64)
    t = np.full((len(n), 1), 41, np.int64)
    asum = ((n + 1) // 2 * 2.0 ** 40 + n // 2 * 3.0 * 2.0 ** -40)[:, None]
    assert not ksn.km_cert(q, t, n, asum).any()
    assert ksn.km_cert(np.array([[40]]), np.array([[41]]), np.array([1]), np.array([[2.0 ** 40]])).all()     # one member passes


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ALL_LAYOUTS)
def test_exact_flags_none_and_special_is_far_from_the_bounds(name, dtype):
    sizes = layout(name)
    a, K, d = ke.assignment(sizes), len(sizes), 3 if name == "lanes" else 17
    X = ke.exact(a, d, dtype)
    assert not ke.predicted_flagged(X, a, K).any() and ke.cert_margin_ok(X, a, K)
    S = ke.special(a, d, dtype)
    assert ke.cert_margin_ok(S, a, K)
    if len(a) >= 5 and d >= 10:
        assert np.isinf(S).sum() == 1 and np.isnan(S).sum() == 1 and (np.signbit(S) & (S == 0)).sum() == 1
        assert ke.predicted_flagged(S, a, K).sum() >= 3              # inf, nan, the huge value (+ the denormal)


def test_flag_block_flags_only_its_columns():
    sizes = ke.LAYOUTS["windows_a1"]
    a, K = ke.assignment(sizes), len(sizes)
    X = ke.flag_block(a, 130, [70])
    fl = ke.predicted_flagged(X, a, K)
    assert fl[:, 70].sum() == sum(s >= 2 for s in sizes) and fl.sum() == fl[:, 70].sum()
    for cols in ([1990], [2049], [1990, 2049]):
        X = ke.flag_block(a, 2050, cols)
        fl = ke.predicted_flagged(X, a, K)
        assert set(np.nonzero(fl.any(axis=0))[0]) == set(cols)
        assert {min(31, j // 64) for j in cols} == {31}             # blocks 31 and 32 share bit 31
    assert ke.cert_margin_ok(X, a, K)


def test_numpy_certify_flag_bit_31():
    # tests/km_shard_np.py: the flag of block >= 31 is bit 31 of an int32
    K, d = 2, 2050
    ops = ksn.NumpyShardSums(np.zeros((0, d)), np.zeros(0, np.int32), K)
    import torch
    q = np.full((K, d), 1 << 30, np.int32)
    t = np.full((K, d), -(1 << 30), np.int32)
    q[1, [70, 1990, 2049]], t[1, [70, 1990, 2049]] = -40, 41
    qt = torch.from_numpy(np.stack([q, -t]))
    asum = torch.from_numpy(np.where(q < 0, 2.0 ** 55, 0.0))
    counts = torch.tensor([5, 40000])
    _, _, flag, mask, nf = ops.certify(torch.zeros((1, K, d), dtype=torch.float64), asum, qt, counts, 1, 0)
    assert flag.dtype == torch.int32 and flag.tolist() == [0, -(1 << 31) | 2] and nf == 3
    assert mask.numpy().sum() == 3 and set(mask.numpy()[1, [70, 1990, 2049]]) == {1}


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("fam", ["exact", "special"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(ke.LAYOUTS))
def test_numpy_reference_matches_the_oracle(name, dtype, fam):
    sizes = ke.LAYOUTS[name]
    a, K, d = ke.assignment(sizes), len(sizes), 17
    X = ke.family(fam, a, d, dtype)
    sums, cnt = ke.ref_sums(X, a, K)
    C = np.random.default_rng(1).standard_normal((K, d))
    Co, co, _ = oracle.kmeans_update(X, a, C, "euclidean", 0.0)
    assert np.array_equal(cnt, co) and np.array_equal(cnt, sizes)
    with np.errstate(all="ignore"):
        mine = np.where(cnt[:, None] != 0, sums / np.maximum(cnt, 1)[:, None], sums)
    assert np.array_equal(mine.view(np.uint64), Co.view(np.uint64))


def test_reference_carry_continues_the_chain():
    sizes = ke.LAYOUTS["windows_a1"]
    a, K = ke.assignment(sizes), len(sizes)
    X = ke.special(a, 17, np.float64)
    whole, cw = ke.ref_sums(X, a, K)
    s1, c1 = ke.ref_sums(X[:1000], a[:1000], K)
    s2, c2 = ke.ref_sums(X[1000:], a[1000:], K, carry=s1)
    assert np.array_equal(s2.view(np.uint64), whole.view(np.uint64)) and np.array_equal(c1 + c2, cw)
