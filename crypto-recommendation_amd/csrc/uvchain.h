// uvchain.h — one 64-term batch of a chain of positive fp64 terms, s_i =
// fl(s_{i-1} + x_i), as integers (uservec.hip's long chains).
//
// s = S u, u = the unit in the last place of s's binade, 2^52 <= S < 2^53. For
// x > 0 with y = x / u no half-integer and S + y < 2^53, fl(s + x) = (S +
// RN(y)) u: the real sum lies in s's binade, whose doubles are the integers
// times u, and S being an integer the rounding depends on y alone. Positive
// terms make the prefix sums monotone, so the last one bounds them all: a batch
// whose terms are all summarised (uv_step's ok) and whose S + sum of RN(y) is at
// most 2^53 - 1 advances s by that integer sum, exactly (uv_advance); any other
// batch is added term by term. kmseg.h makes the same argument for terms of
// either sign (KsStep and its 1.5 * 2^52 shifter are reused here); the lower
// bound it also checks cannot be crossed by positive terms, and a start value
// of exactly 2^52 units is fine: the real sum is above it.
//
// Checked on the host against the plain chain by tests/uvchain_check.cpp.
#pragma once
#include "kmseg.h"

namespace lshkm {

// The biased exponent of s where a batch may be summarised (a positive normal
// s away from both ends of the range, ks_key's bounds), else 0.
KS_HD int uv_binade(double s) {
    const uint64_t b = ks_bits(s);
    const int be = (int)((b >> 52) & 2047u);
    return (b >> 63) || be < 24 || be > 2040 ? 0 : be;
}

// RN(x / u) for the binade be. ok: x / u < 2^51 (false for inf) and no tie.
KS_HD KsStep uv_step(double x, int be) {
    KsStep t;
    const double y = ldexp(x, 52 - (be - 1023));       // exact (power-of-two scaling)
    t.r = KS_ADD(KS_ADD(y, 0x1.8p52), -0x1.8p52);
    t.ok = y < 0x1p51 && fabs(KS_ADD(y, -t.r)) != 0.5;
    return t;
}

// s += total u when the result stays inside the binade; false: s is unchanged.
KS_HD bool uv_advance(double& s, int be, uint64_t total) {
    const uint64_t mant = (1ull << 52) - 1ull;
    const uint64_t S = (ks_bits(s) & mant) | (1ull << 52);
    if (S + total > (1ull << 53) - 1ull) return false;
    const uint64_t nb = ((uint64_t)be << 52) | ((S + total) & mant);
    memcpy(&s, &nb, 8);
    return true;
}

}  // namespace lshkm
