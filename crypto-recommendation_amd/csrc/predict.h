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

}  // namespace lshkm
