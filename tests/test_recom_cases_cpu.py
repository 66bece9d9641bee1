"""Host checks of tests/recom_cases.py: the oracle runs on every case, equals
the plain restatements (long-double cosine, Python Lomuto) on the exact-square
families, and each case has the property that makes it mean something on the
GPU (tests/test_gpu_recom_edges.py): the planted tie sits at its ranks and in
its lanes and nowhere else, the replay's answer differs from "first position
wins", the near tie is near and unequal, every special value comes out."""
import numpy as np
import pytest

import oracle
import recom_cases as rc
from recom_cases import bits

x87 = pytest.mark.skipif(not rc.have_x87(), reason="np.longdouble is not the 80-bit x87 format here")

_ORACLE = {}


def oracle_of(label):
    """(idx, sim, cnt, top) of the oracle, once per case."""
    if label not in _ORACLE:
        X, xm, U, um, up, ui, cp, ci, P, NT = rc.case(label)
        idx, sim, cnt = oracle.p_closest(X, U, cp, ci, P)
        top = oracle.top_n_recom(X, xm, U, um, up, ui, idx, sim, cnt, NT)
        _ORACLE[label] = (idx, sim, cnt, top)
    return _ORACLE[label]


@pytest.mark.parametrize("label", list(rc.CASES))
def test_oracle_runs(label):
    X, xm, U, um, up, ui, cp, ci, P, NT = rc.case(label)
    idx, sim, cnt, top = oracle_of(label)
    N, d = X.shape
    nq = len(U)
    assert N <= 1100 and P >= 1 and U.shape[1] == d and xm.shape == (N,) and um.shape == (nq,)
    assert cp.shape == (nq + 1,) and up.shape == (nq + 1,) and cp[0] == 0 and up[0] == 0
    assert ci.dtype == np.int32 and ui.dtype == np.int32 and len(ci) == cp[-1] and len(ui) == up[-1]
    n = np.diff(cp)
    assert n.min() >= 0 and n.max() <= 1100
    assert len(ci) == 0 or (ci.min() >= 0 and ci.max() < N)       # every list holds valid rows
    assert len(ui) == 0 or (ui.min() >= 0 and ui.max() < d)
    assert np.array_equal(cnt, np.minimum(n, P))
    assert idx.shape == (nq, P) and top.shape == (nq, NT)
    for q in range(min(nq, 400)):
        lst = ci[cp[q]:cp[q + 1]]
        assert len(set(lst.tolist())) == len(lst)                  # no row twice in a list
        assert set(idx[q, :cnt[q]].tolist()) <= set(lst.tolist())


def _sample(label, nq):
    if nq <= 400:
        return np.arange(nq)
    rng = np.random.default_rng(1)
    return np.unique(np.concatenate([np.arange(50), np.arange(nq - 50, nq), rng.integers(0, nq, 200)]))


@x87
@pytest.mark.parametrize("label", rc.EXACT_SQUARE)
def test_oracle_equals_restatement(label):
    """get_P_closest of the oracle against the long-double cosine and the Python
    Lomuto, bit for bit (the two large grid cases: 300 of their users)."""
    X, xm, U, um, up, ui, cp, ci, P, NT = rc.case(label)
    idx, sim, cnt, _ = oracle_of(label)
    qs = _sample(label, len(U))
    sub_cp, sub_ci = rc.csr([ci[cp[q]:cp[q + 1]] for q in qs])
    ridx, rsim, rcnt = rc.p_closest_np(X, U[qs], sub_cp, sub_ci, P)
    assert np.array_equal(rcnt, cnt[qs])
    assert np.array_equal(ridx, idx[qs]), np.nonzero((ridx != idx[qs]).any(axis=1))[0][:8]
    assert np.array_equal(bits(rsim), bits(sim[qs]))


# ------------------------------------------------------------------ len / grid
@pytest.mark.parametrize("label", list(rc.LEN))
def test_len_lengths(label):
    X, xm, U, um, up, ui, cp, ci, P, NT = rc.case(label)
    want = sorted(set([0, 1, 2, P - 1, P, P + 1, P + 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 514, 577, 1025]))
    assert sorted(np.diff(cp).tolist()) == want
    idx, sim, cnt, _ = oracle_of(label)
    if X.shape[1] == 1:
        assert set(np.unique(np.abs(sim[idx >= 0])).tolist()) == {1.0}      # every similarity is +1 or -1
    else:
        for q in range(len(U)):            # distinct similarities
            assert len(np.unique(sim[q, :cnt[q]])) == cnt[q]


def test_len_table_is_the_issue():
    assert rc.LEN_P == [1, 2, 20, 63, 64, 65, 511, 512, 600]
    assert {f"len-P{P}-d24" for P in rc.LEN_P} <= set(rc.LEN)
    assert {"len-P20-d1", "len-P20-d300", "len-P512-d1", "len-P512-d300"} <= set(rc.LEN)
    # P > n, and P + 1 beyond the register limit with lists inside it
    assert max(rc.LEN_P) + 1 > rc.REG_MAX and 511 in rc.len_lengths(600)


def test_grid_lengths():
    assert rc.GRID_NQ == [1, 3, 4, 5, 32773, 70000]
    for nq in rc.GRID_NQ:
        X, xm, U, um, up, ui, cp, ci, P, NT = rc.case(f"grid-nq{nq}")
        assert len(U) == nq and X.shape[1] == 4
        n = np.diff(cp)
        if nq == 70000:
            assert P == 1 and (n == 2).all() and nq > rc.GRID_REPLAY
        else:
            assert n.min() >= 0 and n.max() == 3 and (nq < 4 or set(n.tolist()) == {0, 1, 2, 3})


def test_grid_second_sweep_is_told_apart():
    """Users 32768 .. 32772 are the second step of the grid-stride loop: each
    has neighbours, and its answer is not that of the user one sweep earlier."""
    idx, sim, cnt, top = oracle_of("grid-nq32773")
    for q in range(rc.GRID_SWEEP, rc.GRID_SWEEP + 5):
        assert cnt[q] >= 1 and not np.array_equal(idx[q], idx[q - rc.GRID_SWEEP])
    assert len({tuple(r) for r in idx[rc.GRID_SWEEP:].tolist()}) == 5


def test_grid_every_user_replays():
    """nq = 70000: both candidates of every user are equal, a tie at ranks
    (P, P + 1). Two equal largest keys stay in list order under the quicksort,
    so there the replay keeps the first; in the triple form (a, a', c), c the
    best and P = 2, it keeps a', the later: not "first position wins"."""
    X, xm, U, um, up, ui, cp, ci, P, NT = rc.case("grid-nq70000")
    idx, sim, cnt, _ = oracle_of("grid-nq70000")
    pair = ci.reshape(-1, 2)
    assert np.array_equal(bits(X[pair[:, 0]]), bits(X[pair[:, 1]]))
    assert P == 1 and (cnt == 1).all()
    assert np.array_equal(idx[:, 0], pair[:, 0])
    assert (pair[:, 0] < pair[:, 1]).any() and (pair[:, 0] > pair[:, 1]).any()
    X, xm, U, um, up, ui, cp, ci, P, NT = rc.case("grid-nq70000-triple")
    idx, sim, cnt, _ = oracle_of("grid-nq70000-triple")
    tri = ci.reshape(-1, 3)
    assert len(U) == 70000 and P == 2 and (cnt == 2).all()
    assert np.array_equal(bits(X[tri[:, 0]]), bits(X[tri[:, 1]]))
    assert np.array_equal(idx[:, 0], tri[:, 2]) and (sim[:, 0] > sim[:, 1]).all()
    assert np.array_equal(idx[:, 1], tri[:, 1])


# ------------------------------------------------------------------ tie
def _sorted_sims(label, q):
    """(similarities of user q's list in list order, the list), restated."""
    X, xm, U, um, up, ui, cp, ci, P, NT = rc.case(label)
    lst = ci[cp[q]:cp[q + 1]]
    return rc.cos_sim_np(X[lst], U[q]), lst


@x87
@pytest.mark.parametrize("P", rc.TIE_P)
def test_tie_planted_and_nothing_else(P):
    label = f"tie-P{P}"
    meta = rc.tie_meta(label)
    seen = set()
    for q, m in enumerate(meta):
        s, lst = _sorted_sims(label, q)
        assert len(lst) == m["n"]
        desc = np.sort(s)[::-1]
        r = m["ranks"]
        # the planted ranks hold one value, the tied rows' own
        group = {float(s[p]) for p in m["pos"]}
        assert len(group) == 1 and [int(lst[p]) for p in m["pos"]] == m["members"]
        assert all(desc[k - 1] == desc[r[0] - 1] for k in r) and float(desc[r[0] - 1]) in group
        # and no other equality among the first P + 2 (or beside the planted ranks)
        top = min(len(desc), max(P + 2, r[-1] + 1))
        eq = {k + 1 for k in range(top - 1) if desc[k] == desc[k + 1]}
        assert eq == set(r[:-1]), (q, m, eq)
        # lane layouts
        p0, p1 = m["pos"][0], m["pos"][1]
        if m["layout"] == "lane":
            assert p0 % 64 == p1 % 64 and abs(p0 - p1) == 64
        elif m["layout"] == "lanes":
            assert len({p % 64 for p in m["pos"]}) == len(m["pos"])
        else:
            assert {p0, p1} == {0, m["n"] - 1}
        seen.add((m["placement"], m["layout"], m["n"]))
    ns = rc.tie_ns(P)
    assert {n for (_, _, n) in seen} == set(ns) and {min(ns), 512} <= set(ns) and {513, 600} <= set(ns)
    for placement in rc.TIE_PLACEMENTS:
        if rc.tie_ranks(placement, P) is None:
            continue
        for layout in rc.TIE_LAYOUTS:
            for n in (512, 513, 600):      # the register path's last size and the streaming path
                assert (placement, layout, n) in seen


def test_tie_replay_is_not_first_position():
    """Placement (P, P + 1): one of the two tied rows is kept at rank P, the
    other dropped. In at least a quarter of these users the quicksort keeps the
    one that stands later in the list: a kernel that skipped the replay and let
    the first position win would fail there."""
    later = total = 0
    for P in rc.TIE_P:
        label = f"tie-P{P}"
        idx, sim, cnt, _ = oracle_of(label)
        for q, m in enumerate(rc.tie_meta(label)):
            if m["placement"] != "P_P1":
                continue
            kept = int(idx[q, P - 1])
            assert kept in m["members"] and len(set(m["members"]) & set(idx[q].tolist())) == 1
            first = m["members"][int(np.argmin(m["pos"]))]
            total += 1
            later += kept != first
    assert total >= 40 and later >= total / 4, (later, total)


@x87
def test_tie_below_P_leaves_plain_order():
    """Placements (P+1, P+2) and (P+2, P+3): the oracle's first P are the plain
    descending order of the similarities."""
    n_users = 0
    for P in rc.TIE_P:
        label = f"tie-P{P}"
        idx, sim, cnt, _ = oracle_of(label)
        for q, m in enumerate(rc.tie_meta(label)):
            if m["placement"] not in ("P1_P2", "P2_P3"):
                continue
            s, lst = _sorted_sims(label, q)
            order = np.argsort(-s, kind="stable")[:P]
            assert np.array_equal(idx[q, :cnt[q]], lst[order])
            assert np.array_equal(bits(sim[q, :cnt[q]]), bits(s[order]))
            n_users += 1
    assert n_users >= 40


@x87
@pytest.mark.parametrize("P", [1, 20])
def test_tie_alleq(P):
    label = f"tie-alleq-P{P}"
    X, xm, U, um, up, ui, cp, ci, _, NT = rc.case(label)
    assert np.diff(cp).tolist() == rc.ALLEQ_N[P] and max(rc.ALLEQ_N[P]) <= 600
    assert {512, 513, 65, P + 2} <= set(rc.ALLEQ_N[P])
    for q in range(len(U)):
        s, lst = _sorted_sims(label, q)
        assert len(np.unique(bits(s))) == 1 and np.isfinite(s[0]) and s[0] != 0


def test_tie_zero_carries_the_sign():
    X, xm, U, um, up, ui, cp, ci, P, NT = rc.case("tie-zero")
    idx, sim, cnt, _ = oracle_of("tie-zero")
    one = oracle.p_closest(X, U[:1], np.array([0, 1], np.int64), np.array([0], np.int32), 1)[1]
    assert bits(one)[0, 0] == rc.NEG_ZERO                        # the issue's row against the issue's user
    kept = bits(sim)[idx >= 0]
    assert (kept == rc.NEG_ZERO).sum() >= 5 and (kept == 0).sum() >= 5
    for q in range(len(U)):                                       # side by side in one user's output
        b = bits(sim[q, :cnt[q]])
        if (b == rc.NEG_ZERO).any() and (b == 0).any():
            break
    else:
        raise AssertionError("no user keeps both zeros")


# ------------------------------------------------------------------ near
def test_near_is_near_and_unequal():
    users = close = 0
    copy_first_pos = copy_first_idx = 0
    for P in rc.NEAR_P:
        label = f"near-P{P}"
        X, xm, U, um, up, ui, cp, ci, _, NT = rc.case(label)
        assert X.shape[1] == 100 and sorted(set(np.diff(cp).tolist())) == sorted({P + 2, 80, 512})
        for q, m in enumerate(rc.near_meta(label)):
            pair = np.array([m["orig"], m["copy"]], np.int32)
            _, s, _ = oracle.p_closest(X, U[q:q + 1], np.array([0, 2], np.int64), pair, 2)
            users += 1
            close += (s[0, 0] != s[0, 1]) and rc.ulps_apart(s[0, 0], s[0, 1]) <= 16
            copy_first_pos += m["pos_copy"] < m["pos_orig"]
            copy_first_idx += m["copy"] < m["orig"]
            # the two are ranks P and P + 1 of the list, or next to them
            full, fs, _ = oracle.p_closest(X, U[q:q + 1], np.array([0, m["n"]], np.int64), ci[cp[q]:cp[q + 1]], P + 1)
            assert {m["orig"], m["copy"]} == set(full[0, P - 1:P + 1].tolist())
    assert users == 3 * 3 * rc.NEAR_REPS
    assert close >= 0.9 * users, (close, users)
    for k in (copy_first_pos, copy_first_idx):
        assert users / 3 <= k <= 2 * users / 3, (k, users)


# ------------------------------------------------------------------ value
@pytest.mark.parametrize("n", [12, 520])
def test_value_classes(n):
    label = f"value-n{n}"
    X, xm, U, um, up, ui, cp, ci, P, NT = rc.case(label)
    idx, sim, cnt, _ = oracle_of(label)
    assert P == n and (np.diff(cp) == n).all() and (cnt == n).all()
    assert (n <= rc.REG_MAX) == (n == 12)
    k, v = rc.VALUE_ROWS.index, rc.VALUE_USERS.index
    assert bits(X[k("pnan")])[rc.VALUE_COL] == rc.INPUT_NAN and bits(X[k("nnan")])[rc.VALUE_COL] == rc.DEFAULT_NAN
    assert np.isnan(X).sum() == 2 and np.isinf(X).sum() == 4
    for q in range(len(U)):
        assert set(range(12)) <= set(idx[q].tolist())            # every special row is kept

    def sim_of(user, row):
        q = v(user)
        return int(bits(sim[q])[np.nonzero(idx[q] == k(row))[0][0]])

    b = bits(sim)
    for cls in (0x7FF0000000000000, 0xFFF0000000000000, 0, rc.NEG_ZERO, rc.DEFAULT_NAN, rc.INPUT_NAN):
        assert (b == cls).any(), hex(cls)
    # which operands give which class
    assert sim_of("plain", "pinf") == rc.DEFAULT_NAN             # inf / inf
    assert sim_of("plain", "bothinf") == rc.DEFAULT_NAN          # inf - inf
    assert sim_of("plain", "zero") == rc.DEFAULT_NAN             # 0 / 0
    assert sim_of("zerocol", "pinf") == rc.DEFAULT_NAN           # inf * 0
    assert sim_of("plain", "pnan") == rc.INPUT_NAN               # an input NaN keeps its sign
    assert sim_of("plain", "nnan") == rc.DEFAULT_NAN
    assert sim_of("zerocol", "pnan") == rc.INPUT_NAN             # NaN * 0
    assert sim_of("plain", "e200") in (0, rc.NEG_ZERO)           # finite / inf
    assert sim_of("plain", "em200") in (0x7FF0000000000000, 0xFFF0000000000000)      # x / 0
    assert sim_of("e200", "em200") == rc.DEFAULT_NAN             # denominator 0 * inf
    for row in ("p450", "m450", "m537"):
        s = np.array([sim_of("plain", row)], np.uint64).view(np.float64)[0]
        assert np.isfinite(s) and s != 0, (row, s)
    for user in ("p450", "m450"):
        s = np.array([sim_of(user, "plain")], np.uint64).view(np.float64)[0]
        assert np.isfinite(s) and s != 0, (user, s)


# ------------------------------------------------------------------ topn
def test_topn_case():
    X, xm, um, up, ui, nb_idx, nb_sim, nb_cnt, plan = rc.topn_case()
    assert len(plan) == len(rc.TOPN_CNT) * len(rc.TOPN_SIMS) * len(rc.TOPN_M) == len(um)
    assert sorted(set(np.diff(up).tolist())) == [0, 1, 63, 64, 65, 130] and X.shape[1] == 130
    assert sorted(set(nb_cnt.tolist())) == [0, 1, rc.TOPN_P]
    assert np.array_equal(X[:, 0:30], X[:, 65:95]) and (X[:, 100:130] == X[:, 100:101]).all()
    assert rc.TOPN_NTOP == [1, 3, 4, 63, 64, 65, 66, 67, 68, 130, 133]
    live = nb_sim[np.arange(nb_sim.shape[1])[None, :] < nb_cnt[:, None]]
    b = bits(live)
    for cls in (rc.INPUT_NAN, rc.DEFAULT_NAN, 0x7FF0000000000000, 0xFFF0000000000000, 0, rc.NEG_ZERO):
        assert (b == cls).any(), hex(cls)
    pred = rc.predicted_np(X, xm, um, up, ui, nb_idx, nb_sim, nb_cnt)
    for q, (c, kind, m) in enumerate(plan):
        p = pred[up[q]:up[q + 1]]
        if c == 0 or kind == "allzero":
            assert np.isnan(p).all()                              # 0 / 0
        if kind == "cancel" and c == rc.TOPN_P:
            assert (p == um[q]).all()                             # the terms cancel: all predictions equal
        if kind == "plain" and c and m == 130:
            assert np.isfinite(p).all() and len(np.unique(p)) < m      # equal predictions among distinct ones
    U = np.zeros((len(um), X.shape[1]))
    for n_top in (1, 65, 133):
        want = oracle.top_n_recom(X, xm, U, um, up, ui, nb_idx, nb_sim, nb_cnt, n_top)
        assert np.array_equal(want, rc.top_n_np(pred, up, ui, n_top)), n_top


# ------------------------------------------------------------------ fixtures
def test_fixture_inputs_are_the_cases():
    assert sorted(rc.FIXTURES) == rc.fixtures()
    fam = sorted(rc.FIXTURES[n].split("-")[0] for n in rc.FIXTURES)
    assert fam == ["len", "near", "tie", "value"] and rc.FIXTURES["recomedge_len"] == "len-P20-d24"
    for name in rc.FIXTURES:
        g = rc.fixture(name)
        c = rc.fixture_inputs(name)
        for key, a in zip(rc.INPUT_KEYS, c[:8]):
            assert g[key].dtype == a.dtype and g[key].shape == a.shape, (name, key)
            same = bits(g[key]) == bits(a) if a.dtype == np.float64 else g[key] == a
            assert np.all(same), (name, key)
