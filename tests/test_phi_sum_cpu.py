"""CPU: the summed phi of one k = 4 table against the term-by-term form.

crypto-recommendation_amd/csrc/tile.h has two forms of a table's EuclideanPhi
sum. phi_term (tile.h, "EuclideanPhi arithmetic") is the general one: temp =
int32(h * r) wrapping, ((temp % M) + M) % M by compares, M = 2^31 - 1; the four
terms are added in uint32 (the sum wraps) and phi_final reduces the sum with
two conditional subtractions. phi_sum4_small (tile.h) is what the fused pass
runs on certified hashes (|h| < 2^22, r in [0, 100], so h * r needs 24-bit
operands only and does not wrap): (p0 + p1 + p2 + p3) - M (s0 + s1 + s2 + s3)
with s = p >> 31, in wrapping uint32, written as sp + ss - (ss << 31). Both
are restated here in numpy, operation for operation, and their uint32 results
(before and after phi_final) must be equal."""
import itertools

import numpy as np

M = np.uint32(2147483647)       # tile.h PHI_M


def phi_term(h, r):
    """tile.h phi_term: v = int32(uint32(h) * uint32(r)); v >= M: v -= M; v < 0: v += M (twice)."""
    with np.errstate(over="ignore"):
        v = (h.astype(np.uint32) * r.astype(np.uint32)).view(np.int32).astype(np.int64)
    v = np.where(v >= int(M), v - int(M), v)
    v = np.where(v < 0, v + int(M), v)
    v = np.where(v < 0, v + int(M), v)
    return v.astype(np.uint32)


def phi_final(hn):
    """tile.h phi_final: two conditional subtractions of M."""
    hn = np.where(hn >= M, hn - M, hn)
    return np.where(hn >= M, hn - M, hn).astype(np.uint32)


def mul24(h, r):
    """__mul24: the low 32 bits of the product of the operands' sign-extended low 24 bits."""
    def sx(v):
        return ((v.astype(np.int64) & 0xFFFFFF) ^ 0x800000) - 0x800000
    return (sx(h) * sx(r)).astype(np.uint64).astype(np.uint32).view(np.int32)


def phi_sum4_small(h, r):
    """tile.h phi_sum4_small; h, r: [n, 4] int32."""
    p = mul24(h, r)
    with np.errstate(over="ignore"):
        sp = p.view(np.uint32).sum(axis=1, dtype=np.uint32)
        ss = (p >> 31).sum(axis=1, dtype=np.int32).view(np.uint32)
        return sp + ss - (ss << np.uint32(31))


def term_by_term(h, r):
    with np.errstate(over="ignore"):
        return phi_term(h, r).sum(axis=1, dtype=np.uint32)


def check(h, r):
    h, r = np.ascontiguousarray(h, dtype=np.int32), np.ascontiguousarray(r, dtype=np.int32)
    want, got = term_by_term(h, r), phi_sum4_small(h, r)
    assert want.dtype == got.dtype == np.uint32
    bad = np.flatnonzero(want != got)
    assert bad.size == 0, (h[bad[:4]], r[bad[:4]], want[bad[:4]], got[bad[:4]])
    assert np.array_equal(phi_final(want), phi_final(got))


H_EDGE = (0, 1, -1, 2 ** 22 - 1, -(2 ** 22 - 1))
R_EDGE = (0, 1, 99, 100)


def test_edges_all_sign_patterns():
    """Every 4-tuple of h in {0, +-1, +-(2^22 - 1)} (all sign patterns of four
    terms among them) with every 4-tuple of r in {0, 1, 99, 100}."""
    hs = np.array(list(itertools.product(H_EDGE, repeat=4)), dtype=np.int32)        # 625
    rs = np.array(list(itertools.product(R_EDGE, repeat=4)), dtype=np.int32)        # 256
    h = np.repeat(hs, len(rs), axis=0)
    r = np.tile(rs, (len(hs), 1))
    check(h, r)
    # the wrap of the uint32 sum is exercised: four terms near M
    big = term_by_term(np.full((1, 4), -1, np.int32), np.full((1, 4), 1, np.int32))
    assert int(big[0]) == (4 * (int(M) - 1)) % 2 ** 32


def test_sign_patterns_random_magnitudes():
    """The 16 sign patterns of four terms, random magnitudes over the whole contract range."""
    rng = np.random.default_rng(20240521)
    n = 4096
    for signs in itertools.product((1, -1), repeat=4):
        h = rng.integers(1, 2 ** 22, size=(n, 4), dtype=np.int64) * np.array(signs)
        r = rng.integers(0, 101, size=(n, 4), dtype=np.int64)
        check(h, r)


def test_random_draws():
    rng = np.random.default_rng(7)
    n = 10 ** 6
    h = rng.integers(-(2 ** 22 - 1), 2 ** 22, size=(n, 4), dtype=np.int64)
    r = rng.integers(0, 101, size=(n, 4), dtype=np.int64)
    check(h, r)


def test_identity_outside_the_contract():
    """p - M (p >> 31) equals the select form p < 0 ? p + M : p for every int32 p,
    so an uncertified h (any value; its phi is rewritten by the fix-up) gives the
    summed form the same bits as tile.h's phi_term_small term by term."""
    rng = np.random.default_rng(11)
    h = rng.integers(-2 ** 31, 2 ** 31, size=(10 ** 5, 4), dtype=np.int64).astype(np.int32)
    r = rng.integers(0, 101, size=(10 ** 5, 4), dtype=np.int64).astype(np.int32)
    p = mul24(h, r)
    with np.errstate(over="ignore"):
        small = np.where(p < 0, p.view(np.uint32) + M, p.view(np.uint32)).sum(axis=1, dtype=np.uint32)
    assert np.array_equal(small, phi_sum4_small(h, r))
