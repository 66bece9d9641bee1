// Host check of crypto-recommendation_amd/csrc/hash_exact.h against the real
// x87 long double: the fp64 decisions (hash_decide_floor / hash_decide_sign)
// may decline, but a value they certify must be the reference's
// int(floorl((ip + t) / w)) / ip >= 0, and the soft-x87 forms (hash_x87_floor /
// hash_x87_sign) must give it always. Cases: random rows; exact grid sums a few
// x87 ulps from an integer and from 0; |y| around 2^31 (the reference's FISTP
// stores INT_MIN outside the int range); inf, NaN and overflowing products.
// Built and run by tests/test_lib_cpu.py. Exit code 0 = no mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../crypto-recommendation_amd/csrc/hash_exact.h"

static const int32_t INDEF = (int32_t)0x80000000;

// int(floorl(q)) as the reference's build computes it
static int32_t ref_floor(long double q) {
    if (!(q >= -2147483648.0L && q < 2147483648.0L)) return INDEF;   // inf / NaN too
    return (int32_t)floorl(q);
}

struct Tally { long cases = 0, bad = 0, declined_floor = 0, declined_sign = 0; };

template <typename TX>
static void check(const std::vector<double>& v, const std::vector<TX>& x, float t, float w, Tally& ta) {
    const int d = (int)v.size();
    volatile double prod;                          // the reference's product, rounded to double
    long double ip = 0.0L, vn2 = 0.0L;
    double acc = 0.0, xn2 = 0.0;
    for (int j = 0; j < d; j++) {
        prod = v[j] * (double)x[j];
        ip += (long double)prod;
        vn2 += (long double)v[j] * (long double)v[j];
        acc = std::fma(v[j], (double)x[j], acc);
        xn2 = std::fma((double)x[j], (double)x[j], xn2);
    }
    const long double q = (ip + (long double)t) / (long double)w;
    const int32_t want_floor = ref_floor(q);
    const bool in_range = q >= -2147483648.0L && q < 2147483648.0L;
    const int want_sign = ip >= 0 ? 1 : 0;
    const double pn = (double)sqrtl(vn2) * (1.0 + 0x1p-40);          // |v| rounded up
    const double P = pn * std::sqrt(xn2) * (1.0 + 0x1p-40);
    const auto proj = [&](int j) { return v[j]; };
    ta.cases++;
    int32_t hv = 0;
    if (hash_decide_floor(acc, P, (double)t, w, d, hv)) {
        // outside the int range nothing may be certified: what the cast of such a
        // double gives differs between machines
        if (hv != want_floor || !in_range) {
            if (ta.bad < 10) fprintf(stderr, "certified floor %d != %d (case %ld)\n", hv, want_floor, ta.cases);
            ta.bad++;
        }
    } else {
        ta.declined_floor++;
    }
    hv = hash_x87_floor(proj, x.data(), d, (double)t, w);
    if (hv != want_floor) {
        if (ta.bad < 10) fprintf(stderr, "x87 floor %d != %d (case %ld)\n", hv, want_floor, ta.cases);
        ta.bad++;
    }
    int bit = 0;
    if (hash_decide_sign(acc, P, d, bit)) {
        if (bit != want_sign) {
            if (ta.bad < 10) fprintf(stderr, "certified sign %d != %d (case %ld)\n", bit, want_sign, ta.cases);
            ta.bad++;
        }
    } else {
        ta.declined_sign++;
    }
    bit = hash_x87_sign(proj, x.data(), d);
    if (bit != want_sign) {
        if (ta.bad < 10) fprintf(stderr, "x87 sign %d != %d (case %ld)\n", bit, want_sign, ta.cases);
        ta.bad++;
    }
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 1000000;
    std::mt19937_64 rng(20260);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    auto grid = [&](int span) { return (double)((long)(rng() % (2 * span + 1)) - span) / 8.0; };
    const float pow2w[4] = {0.25f, 0.5f, 1.f, 2.f};
    Tally ta;
    for (long it = 0; it < n; it++) {
        const int kind = (int)(it % 8);
        const int d = 4 + (int)(rng() % 29);
        std::vector<double> v(d);
        std::vector<float> x(d);
        float t, w;
        if (kind < 3) {                            // random rows, random scale
            const double sc = kind == 2 ? std::ldexp(1.0, (int)(rng() % 60) - 30) : 1.0;
            for (int j = 0; j < d; j++) { v[j] = (double)(float)u(rng); x[j] = (float)(u(rng) * sc); }
            w = (float)(0.05 + std::fabs(u(rng)) * 4.0);
            t = (float)(std::fabs(u(rng)) * w);
        } else if (kind < 6) {
            // exact sums on the 1/64 grid (kind 4: cancelling to 0), one or two
            // products of ~2^-60 on top: a few x87 ulps from an integer / from 0
            for (int j = 0; j < d; j++) { v[j] = grid(24); x[j] = (float)grid(24); }
            if (kind == 4)
                for (int j = 0; j + 1 < d; j += 2) { v[j + 1] = v[j]; x[j + 1] = -x[j]; }
            if (kind == 4 && (d & 1)) x[d - 1] = 0.f;
            const int tiny = (int)(rng() % 3);
            for (int q = 0; q < tiny; q++) {
                const int j = (int)(rng() % d);
                v[j] = std::ldexp((double)(1 + rng() % 7), -30 - (int)(rng() % 4)) * (rng() & 1 ? 1 : -1);
                x[j] = (float)std::ldexp((double)(1 + rng() % 7), -30 - (int)(rng() % 4));
            }
            w = pow2w[rng() % 4];
            t = kind == 4 ? 0.f : (float)((double)(rng() % 16) / 8.0);
        } else if (kind == 6) {
            // |y| around 2^31, both signs: one term of +-2^31 w, the rest small
            w = pow2w[rng() % 4];
            for (int j = 0; j < d; j++) { v[j] = grid(8); x[j] = (float)grid(8); }
            v[0] = rng() & 1 ? 1.0 : -1.0;
            x[0] = (float)std::ldexp((double)w, 31) * (rng() % 4 == 0 ? 1.0000001f : 1.f);
            if (rng() % 8 == 0) x[0] *= 3.7f;
            t = (float)((double)(rng() % 16) / 8.0);
        } else {
            // inf / NaN inputs and huge finite ones
            for (int j = 0; j < d; j++) { v[j] = (double)(float)u(rng); x[j] = (float)u(rng); }
            const int what = (int)(rng() % 5);
            const int j = (int)(rng() % d), j2 = (int)(rng() % d);
            if (what == 0) x[j] = std::numeric_limits<float>::infinity();
            if (what == 1) x[j] = -std::numeric_limits<float>::infinity();
            if (what == 2) x[j] = std::numeric_limits<float>::quiet_NaN();
            if (what == 3) { x[j] = std::numeric_limits<float>::infinity(); x[j2] = -x[j]; v[j2] = v[j] = 0.5; }
            if (what == 4) for (int q = 0; q < d; q++) x[q] = 3e38f;
            w = (float)(0.05 + std::fabs(u(rng)) * 4.0);
            t = (float)(std::fabs(u(rng)) * w);
        }
        check(v, x, t, w, ta);
        if (kind == 7 && it % 16 == 7) {           // fp64 rows: products that overflow to inf
            std::vector<double> xd(x.begin(), x.end());
            xd[0] = 1e200; v[0] = rng() & 1 ? 1e200 : -1e200;
            if (rng() & 1) { xd[1] = 1e200; v[1] = -v[0]; }
            check(v, xd, t, w, ta);
        }
    }
    printf("cases=%ld bad=%ld declined: floor %.4f%% sign %.4f%%\n", ta.cases, ta.bad,
           100.0 * (double)ta.declined_floor / (double)ta.cases, 100.0 * (double)ta.declined_sign / (double)ta.cases);
    return ta.bad ? 1 : 0;
}
