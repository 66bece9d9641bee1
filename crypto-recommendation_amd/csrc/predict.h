// predict.h — get_predicted_user_sim (lib/crypto_rec.hpp:280-306) at one
// unknown index over a user's kept neighbours: the device function shared by
// get_top_N_recom (recom.hip) and lshkm_predicted_scores (crossval.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lshkm {

// main_sum and abs_sum run over the neighbours in their sorted order
// (:289-297), both from 0.0; the result is main_sum / abs_sum + the user's
// known mean (:299-300). nb_idx / nb_sim: the user's cnt kept neighbours
// (dataset rows of X [.][d] with means x_mean) and their similarities.
__device__ inline double rc_predict_at(const double* __restrict__ X, const double* __restrict__ x_mean, int d,
                                       const int32_t* __restrict__ nb_idx, const double* __restrict__ nb_sim, int cnt,
                                       int index, double um) {
    double main_sum = 0.0, abs_sum = 0.0;
    for (int i = 0; i < cnt; i++) {
        const double cs = nb_sim[i];
        abs_sum = __dadd_rn(abs_sum, fabs(cs));
        const int32_t r = nb_idx[i];
        main_sum = __dadd_rn(main_sum, __dmul_rn(cs, __dsub_rn(X[(int64_t)r * d + index], x_mean[r])));
    }
    return __dadd_rn(__ddiv_rn(main_sum, abs_sum), um);
}

// r = a op b as SSE rounds it when NaNs are about: a NaN operand comes back
// quieted with its own sign and payload (the first operand's if both are NaN);
// a NaN made from other operands (0/0, inf - inf, inf * 0) is the default NaN,
// sign set.
__device__ inline double rc_sse_nan(double a, double b, double r) {
    if (a != a) return __longlong_as_double(__double_as_longlong(a) | 0x0008000000000000ll);
    if (b != b) return __longlong_as_double(__double_as_longlong(b) | 0x0008000000000000ll);
    return r != r ? __longlong_as_double((long long)0xFFF8000000000000ull) : r;
}

// rc_predict_at's value where it is NaN, with the bits the reference's SSE
// chain gives: every operation in the source's operand order (abs_sum + |cs|,
// cs * (x - mean), main_sum + term, main / abs, + um). Users without
// neighbours and all-zero similarities give 0/0, the default NaN; a NaN
// similarity or mean comes through with its own sign. Exact while at most one
// distinct NaN meets an operation (with two, the compiler's choice of the
// first operand decides in the reference, which is not restated). Out of line:
// only NaN predictions come here.
__device__ __noinline__ double rc_predict_nan(const double* __restrict__ X, const double* __restrict__ x_mean, int d,
                                              const int32_t* __restrict__ nb_idx, const double* __restrict__ nb_sim,
                                              int cnt, int index, double um) {
    double main_sum = 0.0, abs_sum = 0.0;
    for (int i = 0; i < cnt; i++) {
        const double cs = nb_sim[i];
        abs_sum = rc_sse_nan(abs_sum, fabs(cs), __dadd_rn(abs_sum, fabs(cs)));
        const int32_t r = nb_idx[i];
        const double xv = X[(int64_t)r * d + index], mv = x_mean[r];
        const double df = rc_sse_nan(xv, mv, __dsub_rn(xv, mv));
        const double term = rc_sse_nan(cs, df, __dmul_rn(cs, df));
        main_sum = rc_sse_nan(main_sum, term, __dadd_rn(main_sum, term));
    }
    const double p = rc_sse_nan(main_sum, abs_sum, __ddiv_rn(main_sum, abs_sum));
    return rc_sse_nan(p, um, __dadd_rn(p, um));
}

}  // namespace lshkm
