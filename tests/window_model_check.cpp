// Host model of the split-f16 tiles' dot products against csrc/tile.h's derived
// bounds (FU_A1H: the hash tile, hash_tile.h hash_tile_step and its callers'
// step additions; FU_A1: the 3-product tile, fused_impl.h tile_mfma):
//   |dot~ - x.v| <= A1 |v||x| + FU_A2 (|v|_1 + |x|_1),
// exact and the norms in long double. The model: x and v split into f16 hi and
// lo parts as the kernels and the host split them; products of f16 values exact
// in f32; inside an MFMA the 16 products and the C operand summed one by one in
// an arbitrary order (as given, reversed, by rising and by falling magnitude,
// shuffled), every one of those additions rounded toward zero, up, down or to
// nearest (one run each: the hardware's rule is not documented). Hash tile: per
// 16-dim step a fresh accumulator takes the lo products, then the hi products;
// the 8 steps are added in f32, round to nearest (VALU adds: what FU_A1H_STEPS
// charges). 3-product tile: acc_hi chains the 8 steps' hi products, acc_lo the
// 16 lo MFMAs; the model returns acc_hi + acc_lo exactly (the users charge that
// addition themselves, 2^-23 |dot~|).
// The converse: some adversarial case must exceed the bound formed with half
// the constant, or the model would be too weak to say anything about it.
// Prints the constants, the largest share of each bound met, "bad=0"; exit 0.
#include <algorithm>
#include <cfenv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../crypto-recommendation_amd/csrc/hash_tile.h"

using namespace lshkm;

static long bad = 0, checked = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        checked++;                                                      \
        if (!(c)) {                                                     \
            if (bad++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
        }                                                               \
    } while (0)

constexpr int D = FU_D;
static const int MODES[4] = {FE_TOWARDZERO, FE_UPWARD, FE_DOWNWARD, FE_TONEAREST};
static const char* const MODE_NAMES[4] = {"zero", "up", "down", "nearest"};
enum Order { AS_GIVEN, REVERSED, RISING, FALLING, SHUFFLED, N_ORDERS };

// one f32 addition under the current rounding mode (volatile: done at run time)
__attribute__((noinline)) static float add_f32(float a, float b) {
    volatile float x = a, y = b;
    volatile float z = x + y;
    return z;
}

struct Split {
    float hi[D], lo[D];
};
// the kernels' split of an fp32 row (tile.h split8_hi: hi = f16(x), lo = f16(x - f32(hi)), the residual exact in f32)
static Split split_row(const float* x) {
    Split s;
    for (int j = 0; j < D; j++) {
        const _Float16 h = (_Float16)x[j];
        s.hi[j] = (float)h;
        s.lo[j] = (float)(_Float16)(x[j] - (float)h);
    }
    return s;
}
// the host's split of a projection (api.cpp ProjTable: fp64 value, the residual through f32) and of a
// centroid (fused_centroid_prep: the value rounded to f32 first)
static Split split_proj(const double* v, bool via_f32) {
    Split s;
    for (int j = 0; j < D; j++) {
        if (via_f32) {
            const float f = (float)v[j];
            const _Float16 h = (_Float16)f;
            s.hi[j] = (float)h;
            s.lo[j] = (float)(_Float16)(f - (float)h);
        } else {
            const _Float16 h = (_Float16)v[j];
            s.hi[j] = (float)h;
            s.lo[j] = (float)(_Float16)(float)(v[j] - (double)(float)h);
        }
    }
    return s;
}

// One MFMA: C and the 16 products a[j] b[j], summed one by one in the given order.
static float mfma16(const float* a, const float* b, float c, int order, int mode, std::mt19937& rng) {
    float t[17];
    for (int j = 0; j < 16; j++) t[j + 1] = a[j] * b[j];      // exact: 11-bit x 11-bit significands
    t[0] = c;
    switch (order) {
        case REVERSED: std::reverse(t, t + 17); break;
        case RISING: std::sort(t, t + 17, [](float p, float q) { return fabsf(p) < fabsf(q); }); break;
        case FALLING: std::sort(t, t + 17, [](float p, float q) { return fabsf(p) > fabsf(q); }); break;
        case SHUFFLED: std::shuffle(t, t + 17, rng); break;
        default: break;
    }
    fesetround(mode);
    float s = t[0];
    for (int j = 1; j < 17; j++) s = add_f32(s, t[j]);
    fesetround(FE_TONEAREST);
    return s;
}

// The hash tile's value of one function for one row.
static float hash_tile_dot(const Split& v, const Split& x, int order, int mode, std::mt19937& rng) {
    float tot = 0.f;
    for (int s = 0; s < 8; s++) {
        const int o = 16 * s;
        float acc = mfma16(v.lo + o, x.hi + o, 0.f, order, mode, rng);
        acc = mfma16(v.hi + o, x.lo + o, acc, order, mode, rng);
        acc = mfma16(v.hi + o, x.hi + o, acc, order, mode, rng);
        tot = s == 0 ? acc : add_f32(tot, acc);                 // VALU add, round to nearest
    }
    return tot;
}
// The 3-product tile's acc_hi + acc_lo, the last addition exact.
static long double tile3_dot(const Split& v, const Split& x, int order, int mode, std::mt19937& rng) {
    float hi = 0.f, lo = 0.f;
    for (int s = 0; s < 8; s++) {
        const int o = 16 * s;
        hi = mfma16(v.hi + o, x.hi + o, hi, order, mode, rng);
        lo = mfma16(v.hi + o, x.lo + o, lo, order, mode, rng);
        lo = mfma16(v.lo + o, x.hi + o, lo, order, mode, rng);
    }
    return (long double)hi + (long double)lo;
}

struct Share {
    double a1h = 0.0, a1 = 0.0;      // largest (|err| - A2 part) / (A1 |v||x|) met
};

// Every order and mode of both tiles on one (v, x); returns the shares of the two bounds.
static Share run_case(const double* v, const float* x, bool v_via_f32, std::mt19937& rng, bool assert_bound) {
    long double exact = 0.0L, nv = 0.0L, nx = 0.0L, v1 = 0.0L, x1 = 0.0L;
    for (int j = 0; j < D; j++) {
        exact += (long double)v[j] * (long double)x[j];
        nv += (long double)v[j] * (long double)v[j];
        nx += (long double)x[j] * (long double)x[j];
        v1 += fabsl((long double)v[j]);
        x1 += fabsl((long double)x[j]);
    }
    const long double vx = sqrtl(nv) * sqrtl(nx), a2 = (long double)FU_A2 * (v1 + x1);
    const Split sv = split_proj(v, v_via_f32), sx = split_row(x);
    Share sh;
    for (int m = 0; m < 4; m++)
        for (int o = 0; o < N_ORDERS; o++) {
            const long double eh = fabsl((long double)hash_tile_dot(sv, sx, o, MODES[m], rng) - exact);
            const long double e3 = fabsl(tile3_dot(sv, sx, o, MODES[m], rng) - exact);
            if (assert_bound) {
                CHECK(eh <= (long double)FU_A1H * vx + a2);
                CHECK(e3 <= (long double)FU_A1 * vx + a2);
            }
            if (vx > 0.0L) {
                sh.a1h = std::max(sh.a1h, (double)((eh - a2) / ((long double)FU_A1H * vx)));
                sh.a1 = std::max(sh.a1, (double)((e3 - a2) / ((long double)FU_A1 * vx)));
            }
        }
    return sh;
}

static void take(Share& into, const Share& s) {
    into.a1h = std::max(into.a1h, s.a1h);
    into.a1 = std::max(into.a1, s.a1);
}

int main(int argc, char** argv) {
    const int nrand = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937 rng(0x5EED);
    std::normal_distribution<double> nd(0.0, 1.0);
    std::uniform_real_distribution<double> ud(0.0, 1.0);
    double v[D];
    float x[D];
    Share rnd, adv;

    // the constants as the sums of their parts (tile.h), against the issue's figures
    CHECK(FU_A1H > 0.79 * 0x1p-18 && FU_A1H < 0.81 * 0x1p-18);
    CHECK(FU_A1 > 1.047 * 0x1p-16 && FU_A1 < 1.06 * 0x1p-16);
    CHECK(FU_A1H_STEPS == 7 * 0x1p-24 && FU_A1H_MFMA == 16 * 0x1p-23 && FU_A1_HI_CHAIN == 128 * 0x1p-23);

    // ---- random full-mantissa vectors, scales 2^-8 .. 2^12, projections fp32 (euclidean) and fp64 (cosine's rows)
    for (int i = 0; i < nrand; i++) {
        const double sx = ldexp(1.0, (int)(i % 21) - 8), sv = i % 3 == 0 ? 1.0 : ldexp(1.0, (int)(i % 7) - 3);
        const bool v32 = i % 2 == 0;
        for (int j = 0; j < D; j++) {
            const double vv = nd(rng) * sv;
            v[j] = v32 ? (double)(float)vv : vv;
            x[j] = (float)(nd(rng) * sx);
        }
        take(rnd, run_case(v, x, i % 4 == 1, rng, true));
    }
    // ---- all terms of one sign (the worst case for the sum of |terms|), x parallel to v in half of them
    for (int i = 0; i < nrand; i++) {
        for (int j = 0; j < D; j++) {
            v[j] = (double)(float)fabs(nd(rng));
            x[j] = i % 2 ? (float)(v[j] * 3.0) : (float)fabs(nd(rng));
            if (i % 4 >= 2) { v[j] = -v[j]; }
        }
        take(rnd, run_case(v, x, false, rng, true));
    }
    // ---- f16 rounding ties and subnormal lo parts: x = h + half an f16 ulp of h (+- one f32 ulp),
    // |x| from the f16 subnormals (2^-24) up; the lo part is subnormal in f16 wherever |x| < 2^-3
    for (int i = 0; i < nrand; i++) {
        for (int j = 0; j < D; j++) {
            const int e = (int)(ud(rng) * 30.0) - 26;                         // 2^-26 .. 2^3
            const float h = (float)(_Float16)(float)ldexp(1.0 + ud(rng), e);
            const float half_ulp = h >= 0x1p-14f ? ldexpf(1.f, ilogbf(h) - 11) : 0x1p-25f;
            float t = h + half_ulp;
            const int k = (int)(ud(rng) * 3.0);
            if (k == 1) t = nextafterf(t, 0.f);
            if (k == 2) t = nextafterf(t, 1e30f);
            x[j] = ud(rng) < 0.5 ? t : -t;
            const float hv = (float)(_Float16)(float)ldexp(1.0 + ud(rng), (int)(ud(rng) * 12.0) - 9);
            const float tv = hv + ldexpf(1.f, ilogbf(hv) - 11);
            v[j] = (double)(i % 2 ? tv : (float)nd(rng)) * (ud(rng) < 0.5 ? 1.0 : -1.0);
        }
        take(rnd, run_case(v, x, i % 4 == 1, rng, true));
    }
    // ---- |x| near FU_RANGE: one large coordinate, or the norm spread over all of them
    for (int i = 0; i < nrand / 2 + 1; i++) {
        for (int j = 0; j < D; j++) {
            v[j] = (double)(float)nd(rng);
            x[j] = i % 2 ? (float)((0.9 + 0.1 * ud(rng)) * 32767.0 / sqrt((double)D)) * (ud(rng) < 0.5 ? 1.f : -1.f)
                         : (float)(nd(rng) * 4.0);
        }
        if (i % 2 == 0) x[(i / 2) % D] = nextafterf(FU_RANGE, 0.f) * 0.999f;
        take(rnd, run_case(v, x, false, rng, true));
    }

    // ---- adversarial (the bound asserted as everywhere, and the converse's material): x = v (Cauchy-Schwarz
    // tight), all values exact in f16 (no lo part), one dominant product a^2 just above a power of two at
    // the head of its step or chain, so that every later addition works at the sum's full magnitude, and
    // small products that each lose nearly a whole ulp of it under one of the modes:
    //   up:      q^2 far below the ulp (each addition rounds a whole ulp up);
    //   zero:    g^2 = 0.9998 ulp (each addition is truncated away);
    //   nearest: the later steps' sums just above half an ulp (the step additions).
    // scale 2^8 keeps the A2 part negligible.
    const double a = 256.0 * (1.0 + 0x1p-10);                 // a^2 = 2^16 (1 + 2^-9 + 2^-20): ulp 2^-7
    const double smalls[3] = {0x1p-14 * 256.0, 0x1p-12 * (1448.0 / 1024.0) * 256.0, 0x1p-24 * 256.0};
    for (int si = 0; si < 3; si++)
        for (int head = 0; head < 2; head++)
            for (int variant = 0; variant < 2; variant++) {
                for (int j = 0; j < D; j++) v[j] = smalls[si];
                if (variant == 1)
                    // steps 1..7: one product of half an ulp of a^2 and 15 far smaller ones: under
                    // round-up the step's sum lands just above the tie of the step addition
                    for (int s = 1; s < 8; s++) {
                        for (int j = 0; j < 16; j++) v[16 * s + j] = 0x1p-24 * 256.0;
                        v[16 * s] = 0x1p-12 * 256.0;
                    }
                v[head ? 15 : 0] = a;
                for (int j = 0; j < D; j++) x[j] = (float)v[j];
                take(adv, run_case(v, x, false, rng, true));
                for (int j = 0; j < D; j++) x[j] = -x[j];
                take(adv, run_case(v, x, false, rng, true));
            }
    // the converse: half the constant is violated by some adversarial case
    CHECK(adv.a1h > 0.5);
    CHECK(adv.a1 > 0.5);
    CHECK(adv.a1h <= 1.0 && adv.a1 <= 1.0 && rnd.a1h <= 1.0 && rnd.a1 <= 1.0);

    printf("FU_A1H=%a (%.4f * 2^-18) FU_A1=%a (%.4f * 2^-16) FU_A2=%a\n", FU_A1H, FU_A1H * 0x1p18, FU_A1, FU_A1 * 0x1p16,
           FU_A2);
    printf("largest share of the bound met: hash tile random %.3f adversarial %.3f; 3-product tile random %.3f "
           "adversarial %.3f (modes:", rnd.a1h, adv.a1h, rnd.a1, adv.a1);
    for (int m = 0; m < 4; m++) printf(" %s", MODE_NAMES[m]);
    printf(")\nchecked=%ld bad=%ld\n", checked, bad);
    return bad ? 1 : 0;
}
