// kpp_chain.h — the arithmetic of k-means++'s prefix chain (k_means_pp,
// lib/clustering_phases/initialization.hpp:118-125), once, for host and device.
//
// The chain s_m = RN(s_{m-1} + q_m), q_m >= 0, is strictly sequential. While s
// stays in one binade [2^e, 2^(e+1)) every s is a multiple of u = 2^(e-52), so
// RN(s + q) = s + u * RN_u(q) unless q is a tie (q / u = k + 1/2, rounded to
// the even s): an integer prefix sum, valid while it stays below 2^53. A chunk
// of KPP_CHUNK rows guesses its binade from an approximate start; a guess only
// chooses the walk's path, never the result. Plain arithmetic, no HIP
// intrinsics: kmeanspp.hip's kernels call these functions, and
// tests/kpp_chain_check.cpp walks them serially against the plain chain.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define KPP_HD __host__ __device__ inline
#else
#define KPP_HD static inline
#endif

namespace lshkm {

constexpr int KPP_CHUNK = 512;                 // rows per chunk
constexpr int KPP_DIRTY = INT_MIN;
constexpr int64_t KPP_TWO53 = 1ll << 53;

struct KppChunk {
    int64_t R;     // sum of the chunk's RN_u(q) in units of 2^(e-52)
    int32_t e;     // guessed binade, or KPP_DIRTY
    int32_t dual;  // 0, or 2048 + the guessed binade eg: prefix arrays in eg, eg + 1
};

// Binade exponent of a positive normal double (s in [2^e, 2^(e+1))); 2^(e+1).
KPP_HD int kpp_binade(double s) {
    uint64_t b;
    memcpy(&b, &s, 8);
    return (int)((b >> 52) & 0x7ff) - 1023;
}
KPP_HD double kpp_binade_end(int e) {
    const uint64_t b = (uint64_t)(e + 1 + 1023) << 52;
    double v;
    memcpy(&v, &b, 8);
    return v;
}
// s (or an approximate start) has a binade the integer form can use (else: 0).
KPP_HD bool kpp_usable(double s) { return s >= 0x1p-900 && s < 0x1p62; }
KPP_HD int kpp_binade0(double s) { return kpp_usable(s) ? kpp_binade(s) : 0; }

// A sum of binade e in units of 2^(e-52) and back (exact); su + r stays in it.
KPP_HD int64_t kpp_to_units(double s, int e) { return (int64_t)ldexp(s, 52 - e); }
KPP_HD double kpp_from_units(int64_t r, int e) { return ldexp((double)r, e - 52); }
KPP_HD bool kpp_fits(int64_t su, int64_t r) { return su + r < KPP_TWO53; }

// RN_u(q) in units of u = 2^(e-52) with its class: 0 resolved, 1 a tie (the
// floor returned: the rounding depends on the running sum's parity), 2 not
// resolvable in binade e (non-finite, q >= 2^(e+1); 0 returned).
KPP_HD int64_t kpp_units(double q, int e, int& cls) {
    if (!(q >= 0.0) || !(q < kpp_binade_end(e))) { cls = 2; return 0; }
    const double t = ldexp(q, 52 - e);          // exact: t < 2^53
    const double r = floor(t);
    const double f = t - r;                     // exact
    cls = f == 0.5 ? 1 : 0;
    return (int64_t)r + (f > 0.5 ? 1 : 0);
}

// A chunk's record from its totals: a its approximate start, next the next
// chunk's (if has_next), t the sum of its rows' units in binade0(a), any the OR
// of their classes. Dirty (the walk stops there): a tie, an unresolvable row,
// an unusable start. Prefix arrays in binades e and e + 1 (dual != 0): a tie,
// or a predicted crossing (the next start lies higher, or t leaves the binade).
KPP_HD KppChunk kpp_chunk_record(double a, bool has_next, double next, int64_t t, int any) {
    const bool usable = kpp_usable(a);
    const int e = kpp_binade0(a);
    const bool cross = usable && (t >= KPP_TWO53 || (has_next && !(next < kpp_binade_end(e))));
    const bool arrays = usable && (cross || (any & 1));
    const bool dirty = !usable || any != 0;
    KppChunk m;
    m.R = dirty ? 0 : t;
    m.e = dirty ? KPP_DIRTY : e;
    m.dual = arrays ? 2048 + e : 0;
    return m;
}

// Prefix-array entries: the inclusive prefix p of RN_u(q) (a tie counted as its
// floor; p < 512 * 2^53 = 2^62) | KPP_TIE if the row itself (class cls) is a
// tie; poison from the first unresolvable row on (bad: their count so far).
constexpr int64_t KPP_TIE = 1ll << 62;
constexpr int64_t KPP_PMASK = KPP_TIE - 1;
constexpr int64_t KPP_POISON = INT64_MIN;
KPP_HD int64_t kpp_entry(int64_t p, int64_t bad, int cls) { return bad ? KPP_POISON : p | (cls == 1 ? KPP_TIE : 0); }
KPP_HD bool kpp_entry_poison(int64_t en) { return en < 0; }
KPP_HD bool kpp_entry_tie(int64_t en) { return (en & KPP_TIE) != 0; }
KPP_HD int64_t kpp_entry_prefix(int64_t en) { return en & KPP_PMASK; }

// The walk's two acceptance rules. A chunk's guess holds for the exact s: s
// usable, in the guessed binade (es = binade0(s)), and s + R still in it.
KPP_HD bool kpp_guess_binade(bool s_ok, int es, const KppChunk& m) { return s_ok && m.e == es; }
KPP_HD bool kpp_guess_holds(double s, const KppChunk& m) {
    const int es = kpp_binade0(s);
    return kpp_guess_binade(kpp_usable(s), es, m) && kpp_fits(kpp_to_units(s, es), m.R);
}
// An entry stops the integer rows begun with su units at prefix base_p:
// unresolvable from here on, a tie, or the sum leaves the binade.
KPP_HD bool kpp_entry_stops(int64_t en, int64_t su, int64_t base_p) {
    return kpp_entry_poison(en) || kpp_entry_tie(en) || !kpp_fits(su, kpp_entry_prefix(en) - base_p);
}

}  // namespace lshkm
