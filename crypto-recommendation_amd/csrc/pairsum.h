// pairsum.h — sums of the reference's exact distances from one member to a
// run of members, in member order: the inner loops shared by the silhouette
// (silhouette.hip: a(i), b(i)) and the PAM medoid update (pam.hip: dist_sum).
// One wave per member i: x_i sits in LDS (broadcast reads); lane L evaluates
// d(x_i, x_j) for member j = jb + L of a 64-member batch, then every lane adds
// the batch's 64 distances in member order (readlane: the sum stays the
// reference's sequential chain).
#pragma once
#include "exact.h"

namespace lshkm {

// x_i (LDS) vs x_j (global), rows of fp32 or fp64: the exact.h order, 4-wide
// loads. The whole wave calls it: the squares go through gp_sq_wave (sq: 64 *
// 16 doubles of wave-private LDS; glibc's pow restated for the few squares
// that need it, batched over the wave -- per lane, a wave paid it in nearly
// every term).
template <typename TX, bool EXSQ>
__device__ inline double sil_euclid(const TX* __restrict__ xi, const TX* __restrict__ xj, int d, double* sq) {
    double acc = 0.0;
    int k = 0;
    if ((d & 3) == 0) {
#pragma unroll 1
        for (; k + 8 <= d; k += 8) {
            double a[4], b[4], df[8], p[8];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                ld4d(xi + k + 4 * h, a);
                ld4d(xj + k + 4 * h, b);
#pragma unroll
                for (int u = 0; u < 4; u++) df[4 * h + u] = __dsub_rn(a[u], b[u]);
            }
            gp_sq_wave<8, sizeof(TX) == 8, EXSQ>(df, p, sq);
#pragma unroll
            for (int u = 0; u < 8; u++) acc = __dadd_rn(acc, p[u]);
        }
        if (k < d) {                                        // d % 8 == 4
            double a[4], b[4], df[4], p[4];
            ld4d(xi + k, a);
            ld4d(xj + k, b);
#pragma unroll
            for (int u = 0; u < 4; u++) df[u] = __dsub_rn(a[u], b[u]);
            gp_sq_wave<4, sizeof(TX) == 8, EXSQ>(df, p, sq);
#pragma unroll
            for (int u = 0; u < 4; u++) acc = __dadd_rn(acc, p[u]);
            k += 4;
        }
    }
#pragma unroll 1
    for (; k < d; k++) {
        const double df[1] = {__dsub_rn((double)xi[k], (double)xj[k])};
        double p[1];
        gp_sq_wave<1, sizeof(TX) == 8, EXSQ>(df, p, sq);
        acc = __dadd_rn(acc, p[0]);
    }
    return sqrt(acc);
}

// sum_{j in [j0, j1)} d(x_i, x_rows[j]) in j order (wave-uniform result);
// lanes past j1 repeat the last member so the whole wave stays in step
template <typename TX, bool EXSQ>
__device__ inline double sil_segment(const TX* __restrict__ xi, const TX* __restrict__ X, int d, int metric,
                                     const int32_t* __restrict__ rows, int64_t j0, int64_t j1, int lane,
                                     double* sq) {
    double acc = 0.0;
    for (int64_t jb = j0; jb < j1; jb += 64) {
        const int64_t j = min<int64_t>(jb + lane, j1 - 1);
        const TX* xj = X + (size_t)rows[j] * d;
        const double dj = metric == 0 ? sil_euclid<TX, EXSQ>(xi, xj, d, sq) : exact_dist(xi, xj, d, metric);
        const int n = (int)min<int64_t>(64, j1 - jb);
        for (int t = 0; t < n; t++) acc = __dadd_rn(acc, __shfl(dj, t));
    }
    return acc;
}

// Two members (same cluster) against the same x_j: each x_j load serves both
// (d % 4 == 0).
template <typename TX, bool EXSQ>
__device__ inline void sil_euclid2(const TX* __restrict__ xa, const TX* __restrict__ xb,
                                   const TX* __restrict__ xj, int d, double& da, double& db, double* sq) {
    double aa = 0.0, ab = 0.0;
    int k = 0;
#pragma unroll 1
    for (; k + 8 <= d; k += 8) {
        double df[16], p[16];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            double b[4], u[4], v[4];
            ld4d(xj + k + 4 * h, b);
            ld4d(xa + k + 4 * h, u);
            ld4d(xb + k + 4 * h, v);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                df[8 * h + 2 * e] = __dsub_rn(u[e], b[e]);
                df[8 * h + 2 * e + 1] = __dsub_rn(v[e], b[e]);
            }
        }
        gp_sq_wave<16, sizeof(TX) == 8, EXSQ>(df, p, sq);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            aa = __dadd_rn(aa, p[2 * e]);
            ab = __dadd_rn(ab, p[2 * e + 1]);
        }
    }
    if (k < d) {                                            // d % 8 == 4
        double b[4], u[4], v[4], df[8], p[8];
        ld4d(xj + k, b);
        ld4d(xa + k, u);
        ld4d(xb + k, v);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            df[2 * e] = __dsub_rn(u[e], b[e]);
            df[2 * e + 1] = __dsub_rn(v[e], b[e]);
        }
        gp_sq_wave<8, sizeof(TX) == 8, EXSQ>(df, p, sq);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            aa = __dadd_rn(aa, p[2 * e]);
            ab = __dadd_rn(ab, p[2 * e + 1]);
        }
    }
    da = sqrt(aa);
    db = sqrt(ab);
}

template <typename TX, bool EXSQ>
__device__ inline void sil_segment2(const TX* __restrict__ xa, const TX* __restrict__ xb,
                                    const TX* __restrict__ X, int d, const int32_t* __restrict__ rows, int64_t j0,
                                    int64_t j1, int lane, double& sa, double& sb, double* sq) {
    double acc_a = 0.0, acc_b = 0.0;
    for (int64_t jb = j0; jb < j1; jb += 64) {
        const int64_t j = min<int64_t>(jb + lane, j1 - 1);
        double da, db;
        sil_euclid2<TX, EXSQ>(xa, xb, X + (size_t)rows[j] * d, d, da, db, sq);
        const int n = (int)min<int64_t>(64, j1 - jb);
        for (int t = 0; t < n; t++) {
            acc_a = __dadd_rn(acc_a, __shfl(da, t));
            acc_b = __dadd_rn(acc_b, __shfl(db, t));
        }
    }
    sa = acc_a;
    sb = acc_b;
}

}  // namespace lshkm
