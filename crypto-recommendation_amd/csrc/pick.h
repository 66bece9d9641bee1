// pick.h -- the listed passes' euclidean pick among a few candidates in the
// reference's exact order: the chains, the group reductions and
// pruned_pick_euclid (the pruned exact pass of exact_pass.hip, and the fused
// refinement's pair rows, fused_refine.hip).
#pragma once
#include "exact.h"

namespace lshkm {

// The reference's euclidean chain with glibc's pow per square, a rolled loop
// inlined where it is used: the kernels' rare exact paths (a call would raise
// the whole kernel to the calling convention's 256 VGPRs).
template <typename TX>
__device__ __attribute__((always_inline)) inline double exact_euclid_rolled(const TX* __restrict__ x,
                                                                            const double* __restrict__ c, int d) {
    double acc = 0.0;
#pragma unroll 1
    for (int j = 0; j < d; j++) acc = __dadd_rn(acc, gp_sq(__dsub_rn((double)x[j], c[j])));
    return sqrt(acc);
}

// The squared euclidean chain of one (row, centroid) pair in the reference's
// order with x*x squares: the reference's value unless pw.hard() afterwards
// (some square pow(x, 2) may round differently, gpow2.h).
template <typename TX>
__device__ inline double euclid_sumsq_mul(const TX* __restrict__ x, const double* __restrict__ c, int d, PwAcc& pw) {
    double acc = 0.0;
    for (int j0 = 0; j0 < d; j0 += 16) {
        double cv[16];
#pragma unroll
        for (int t = 0; t < 16; t++) cv[t] = j0 + t < d ? c[j0 + t] : 0.0;
#pragma unroll
        for (int t = 0; t < 16; t++)
            if (j0 + t < d) {
                const double df = __dsub_rn((double)x[j0 + t], cv[t]);
                const double p = __dmul_rn(df, df);
                pw.add<true>(df);
                acc = __dadd_rn(acc, p);
            }
    }
    return acc;
}

// (best, bi) over a group of G lanes (xor offsets < G): the smallest value, the
// first index on ties (assignment.hpp:66-69 strict '<' in index order); bi < 0:
// no candidate in the lane.
template <int G>
__device__ inline void group_argmin(double& best, int& bi) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        const bool take = oi >= 0 && (bi < 0 || ob < best || (ob == best && oi < bi));
        if (take) { best = ob; bi = oi; }
    }
}
template <int G>
__device__ inline double group_min(double v) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}

// The pruned pass's euclidean pick among a group's candidates (lane: centroid c,
// or c < 0). The chains run with x*x squares; where one of the group holds a
// square pow may round differently (PwAcc), each chain is within 2^-43 of the
// reference's (both sums' roundings, <= gamma_255 of the non-negative terms, plus
// one ulp per square), so the x*x winner stands when every other candidate's sum
// exceeds its own by 2^-41 relative -- the reference's sums then order the same
// way and their square roots are distinct doubles. Otherwise every chain is
// redone with pow (gp_sq). exact_dist (LSHKM_DIST_EXACT): the winner's distance
// from its pow chain; certified mode keeps the x*x one (2^-44 relative).
template <int G, typename TX>
__device__ inline void pruned_pick_euclid(const TX* __restrict__ xr, const double* __restrict__ C, int d, int c,
                                          bool exact_dist, double& best, int& bi) {
    PwAcc pw;
    const double S = c >= 0 ? euclid_sumsq_mul(xr, C + (size_t)c * d, d, pw) : 0.0;
    const bool hard = c >= 0 && pw.hard();
    best = c >= 0 ? sqrt(S) : 0.0;
    bi = c;
    group_argmin<G>(best, bi);
    int anyh = hard ? 1 : 0;
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) anyh |= __shfl_xor(anyh, off);
    if (!anyh) return;                                           // every chain is pow's
    const double S1 = group_min<G>(c >= 0 && c == bi ? S : __builtin_inf());
    const double S2 = group_min<G>(c >= 0 && c != bi ? S : __builtin_inf());
    if (S2 != __builtin_inf() && !(S2 - S1 > 0x1p-41 * S2)) {      // S2 = inf: the lone candidate
        // too close to call: the reference's chains
        best = c >= 0 ? exact_euclid_rolled(xr, C + (size_t)c * d, d) : 0.0;
        bi = c;
        group_argmin<G>(best, bi);
        return;
    }
    if (!exact_dist) return;
    const int w = bi;
    double v = __builtin_inf();
    if (c == w) v = hard ? exact_euclid_rolled(xr, C + (size_t)c * d, d) : best;
    best = group_min<G>(v);
}

// The every-centroid loop of one row over the wave's lanes, dd(c) the
// reference's distance. assignment.hpp:66: the -1 sentinel takes centroid 0's
// distance even if NaN (a zero vector under cosine), which then blocks every
// later '<'; any other NaN is never taken.
template <typename F>
__device__ inline void every_centroid(int K, F&& dd, double& best, int& bi) {
    for (int c = threadIdx.x & 63; c < K; c += 64) {
        const double v = dd(c);
        if (bi < 0 ? (v == v || c == 0) : v < best) { best = v; bi = c; }
    }
}

// The wave's (best, bi) of one row to its outputs: the smallest value, then the
// smallest index (= the first strict minimum in c order); no lane took any:
// the reference's sentinel.
__device__ inline void wave_store(double best, int bi, int64_t row, int32_t* __restrict__ assign,
                                  double* __restrict__ dist) {
    group_argmin<64>(best, bi);
    if ((threadIdx.x & 63) == 0) {
        assign[row] = bi < 0 ? 0 : bi;
        dist[row] = bi < 0 ? -1.0 : best;
    }
}

}  // namespace lshkm
