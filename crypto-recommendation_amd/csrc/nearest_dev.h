// nearest_dev.h — the device helpers lshkm_min_vector_dist (nearest.hip) and
// lshkm_knn (knn.hip) share: the bound constants of DESIGN.md §5f, the
// order-preserving key of a float, and the reference's distance of one (query,
// row) pair.
#pragma once
#include "../../include/lshkm.h"
#include "common.h"
#include "exact.h"

namespace lshkm {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// The part of the cosine radius every pair shares (§5f): the MFMA chain
// ((DP + 8) 2^-24 of |x^||q^|), the reference's own roundings (2^-40), the f32
// roundings of 1/|x^|, 1/|q^|, g~ inv inv, 1 - s~, E, lo and hi (< 2^-21;
// charged 2^-20).
template <int DP> constexpr float nearest_e0_cos() {
    return (float)(((DP + 8) * 0x1p-24 + 0x1p-20 + 0x1p-40) * (1.0 + 0x1p-20));
}
// The euclidean radius is c (|q^|^2 + |x^|^2): 2 (DP + 8) 2^-24 |q^||x^| <=
// (DP + 8) 2^-24 S for the chain, 2^-24 S for the f32 norms, 2^-24 S for their
// sum, 2^-23 S for the fmaf, 3 2^-24 S for E, lo and hi: DP + 15 units, DP + 24
// charged; 2^-40 S covers the reference chain's roundings ((d + 4) 2^-53 of a
// sum <= 2 S (1 + 2^-11)) and the 2^-50 relative margin its sqrt needs.
template <int DP> constexpr float nearest_c1_euc() {
    return (float)(((DP + 24) * 0x1p-24 + 0x1p-40) * (1.0 + 0x1p-20));
}

// Order-preserving key of a non-NaN float.
__device__ inline uint32_t nearest_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The reference's distance from query q (`this`) to row x. Cosine: the x87
// inner product of the double products and 1 - double(ip / denom), with the
// x87's results for special operands as rc_cos_sim (recom.hip) states them: the
// soft chain takes finite products only. On fp64 values qn / xn = the query's /
// row's sequential sum of squares (rc_norm_kernel; glibc's pow restatement and
// the x87 chain in one kernel do not fit the scalar registers); fp32 values
// square exactly and form both sums here.
template <typename T, int METRIC> constexpr bool nearest_wants_norms() {
    return METRIC == LSHKM_METRIC_COSINE && sizeof(T) == 8;
}
template <typename T, int METRIC>
__device__ inline double nearest_dist(const T* __restrict__ q, const T* __restrict__ x, int d, double qn, double xn) {
    if constexpr (METRIC == LSHKM_METRIC_COSINE) {
        X87acc ip;
        ip.init();
        int inf = 0;                             // 1 = a +inf product, 2 = a -inf one
        bool nan = false;
        double a = 0.0, b = 0.0;
        for (int j = 0; j < d; j++) {
            const double qj = (double)q[j], xj = (double)x[j];
            const double p = __dmul_rn(qj, xj);
            if (fabs(p) < __builtin_inf()) ip.add(p);
            else if (p != p) nan = true;
            else inf |= p > 0.0 ? 1 : 2;
            if constexpr (sizeof(T) == 4) {
                a = __dadd_rn(a, __dmul_rn(qj, qj));
                b = __dadd_rn(b, __dmul_rn(xj, xj));
            }
        }
        if constexpr (sizeof(T) == 8) {
            a = qn;
            b = xn;
        }
        const double denom = __dmul_rn(sqrt(a), sqrt(b));
        double quot;
        if (inf || nan || !(denom < __builtin_inf())) {
            const double indefinite = __longlong_as_double((long long)0xFFF8000000000000ull);
            if (nan || inf == 3 || denom != denom) quot = indefinite;
            else if (inf) quot = denom == __builtin_inf() ? indefinite : inf == 1 ? __builtin_inf() : -__builtin_inf();
            else quot = ip.value().s ? -0.0 : 0.0;           // finite / inf
        } else {
            quot = x87_quot(ip.value(), denom);
        }
        return one_minus(quot);
    } else {
        return exact_dist(q, x, d, METRIC);
    }
}

}  // namespace lshkm
