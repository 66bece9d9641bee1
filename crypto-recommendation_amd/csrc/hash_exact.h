// hash_exact.h — the exact value of one hash function from the exact row, for
// every kernel that computes or repairs one; host-callable like softx87.h
// (tests/hash_cert_check.cpp: against real long double). The reference sums
// double-rounded products in x87 long double. The fp64 FMA
// chain acc of the d products (any order) differs from it by at most (d + 2)
// 2^-52 (P + |t|), P >= |v||x| (+ d 2^-1075 for subnormal products of fp64
// rows: the 2^-1000 term); y = (acc + t) / w adds 2^-51 |y|. hash_decide_*
// certify the floor / sign inside that window; hash_x87_* recompute what they
// decline with the soft-x87 chain, bit for bit what the reference computes.
#pragma once
#include <math.h>
#include "softx87.h"

// int(floorl((ip + t) / w)) in fp64: only inside the int range (outside it the
// reference's FISTP stores INT_MIN: the x87 form's); inf / NaN never pass.
SX_HD bool hash_decide_floor(double acc, double P, double tt, float w, int d, int32_t& v) {
    const double ww = (double)w;
    const double y = (acc + tt) / ww;
    const double B = ((double)(d + 2) * 0x1p-52 * (P + fabs(tt)) + 0x1p-1000) / ww + fabs(y) * 0x1p-51;
    const double lo = floor(y - B), hi = floor(y + B);
    if (!(lo == hi && fabs(lo) < 0x1p31)) return false;
    v = (int32_t)lo;
    return true;
}

// ip >= 0 decided in fp64; finite only (no product overflowed).
SX_HD bool hash_decide_sign(double acc, double P, int d, int& v) {
    const double B = (double)(d + 3) * 0x1p-52 * P + 0x1p-1000;
    if (acc > B && acc < 0x1p1000) { v = 1; return true; }
    if (acc < -B && acc > -0x1p1000) { v = 0; return true; }
    return false;
}

// The reference's chain (cust_vector.hpp:117-118): the products rounded to double
// (nothing here can fuse them), summed in x87 order; proj(j) is projection value j.
template <typename PROJ, typename TX>
SX_MD SxSum hash_x87_ip(PROJ proj, const TX* x, int d) {
    SxSum s;
    s.init();
    for (int j = 0; j < d; j++) s.add(proj(j) * (double)x[j]);
    return s;
}
// EuclideanHGen::generate (euclidean_h_gen.hpp:75) and CosineHGen::generate over that chain
template <typename PROJ, typename TX>
SX_MD int32_t hash_x87_floor(PROJ proj, const TX* x, int d, double tt, float w) {
    return sx_hash_floor(hash_x87_ip(proj, x, d), tt, w);
}
template <typename PROJ, typename TX>
SX_MD int hash_x87_sign(PROJ proj, const TX* x, int d) {
    return sx_hash_sign(hash_x87_ip(proj, x, d));
}
