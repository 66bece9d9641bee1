// crossval.hip — the device side of the recommender's 10-fold validation
// (main.cpp:393-437, lsh_rec_10_fold_validation_A) on gfx950:
//   hide_one_score          lib/crypto_rec.hpp:393-449  cv_hide_kernel
//   merge_except_for        lib/crypto_rec.hpp:370-390  cv_excl_* (fold exclusion)
//   get_predicted_user_sim  lib/crypto_rec.hpp:280-306  cv_predict_kernel
//   the ordered error sum   main.cpp:419-429            cv_fold_sum_kernel
// Rows are fp64 user vectors. The ten folds run over one working matrix in
// split order (api_recom.cpp, lshkm_lsh_validate10): the held-out fold is a
// contiguous row range, dropped from a query's ascending result here.
#include "../../include/lshkm.h"
#include "common.h"
#include "kernels.h"
#include "exact.h"
#include "predict.h"

namespace lshkm {

// Row rows[m] (rows == NULL: row m) of X and its mean into W / w_mean.
__global__ __launch_bounds__(256) void cv_gather_kernel(const double* __restrict__ X,
                                                        const double* __restrict__ x_mean,
                                                        const int32_t* __restrict__ rows, int64_t M, int d,
                                                        double* __restrict__ W, double* __restrict__ w_mean) {
    const int64_t total = M * d;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t m = t / d;
        const int j = (int)(t - m * d);
        const int64_t r = rows ? rows[m] : m;
        W[t] = X[r * d + j];
        if (j == 0) w_mean[m] = x_mean[r];
    }
}

// hide_one_score (crypto_rec.hpp:393-449), one thread per user, user m = row
// rows[m] of X (rows == NULL: row m):
//   known_count = d - |unknown set| < 2: false, nothing changed (:405-406);
//   hide_index = draw % known_count, used as a dimension index as it is
//   (:411-412), old_score read before the zeroing; every unknown index set to
//   0 (:415-416); new_mean = the sum from 0.0 of the other d - 1 entries in
//   index order (:419-430); all of them == 0: false, the zeroing stays, mean
//   and unknown set as they were (:432-433); else the mean replaces the hidden
//   entry and becomes the known mean (:436-446).
// hide_idx = -1 where the function returned false; old = 0.0 (main.cpp:409's
// initial value) where it returned before writing *old_score.
__global__ __launch_bounds__(256) void cv_hide_kernel(const double* __restrict__ X, const double* __restrict__ x_mean,
                                                      const int32_t* __restrict__ rows, int64_t M, int d,
                                                      const int64_t* __restrict__ unk_ptr,
                                                      const int32_t* __restrict__ unk_idx,
                                                      const int32_t* __restrict__ draw, double* H,
                                                      double* __restrict__ h_mean, int32_t* __restrict__ hide_idx,
                                                      double* __restrict__ old) {
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
        const int64_t r = rows ? rows[m] : m;
        const double* x = X + r * d;
        double* h = H + m * d;
        for (int j = 0; j < d; j++) h[j] = x[j];
        const int64_t o = unk_ptr[r];
        const int nu = (int)(unk_ptr[r + 1] - o);
        const int known = d - nu;
        h_mean[m] = x_mean[r];
        hide_idx[m] = -1;
        old[m] = 0.0;
        if (known < 2) continue;
        const int hide = (int)((unsigned int)draw[m] % (unsigned int)known);
        old[m] = x[hide];
        for (int e = 0; e < nu; e++) {
            const int idx = unk_idx[o + e];
            if (idx >= 0 && idx < d) h[idx] = 0.0;
        }
        double sum = 0.0;
        bool useless = true;
        for (int j = 0; j < d; j++) {
            if (j == hide) continue;
            const double v = h[j];
            sum = __dadd_rn(sum, v);
            if (v != 0.0) useless = false;
        }
        if (useless) continue;
        const double mean = __ddiv_rn(sum, (double)(d - 1));
        h[hide] = mean;
        h_mean[m] = mean;
        hide_idx[m] = hide;
    }
}

// Fold exclusion over a filled query result (ascending rows per query): the
// members in [lo, hi) form one run [a, b) of the segment. cnt[q] = members kept.
__global__ __launch_bounds__(256) void cv_excl_count_kernel(const int64_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ idx, int64_t nq, int32_t lo,
                                                            int32_t hi, int64_t* __restrict__ cnt,
                                                            int32_t* __restrict__ run_a, int32_t* __restrict__ run_b) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        const int64_t o = ptr[q];
        const int n = (int)(ptr[q + 1] - o);
        auto lower = [&](int32_t v) {           // the first position with idx >= v
            int l = 0, h = n;
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (idx[o + mid] < v) l = mid + 1; else h = mid;
            }
            return l;
        };
        const int a = lower(lo), b = lower(hi);
        run_a[q] = a;
        run_b[q] = b;
        cnt[q] = n - (b - a);
    }
}

// Exclusive prefix offsets of cnt[0 .. nq) into out_ptr[0 .. nq] (one block:
// every thread sums a contiguous chunk, the chunk sums are scanned in LDS).
constexpr int CV_SCAN_T = 1024;
__global__ __launch_bounds__(CV_SCAN_T) void cv_excl_scan_kernel(const int64_t* __restrict__ cnt, int64_t nq,
                                                                 int64_t* __restrict__ out_ptr) {
    __shared__ int64_t part[CV_SCAN_T];
    const int t = threadIdx.x;
    const int64_t chunk = (nq + CV_SCAN_T - 1) / CV_SCAN_T;
    const int64_t b = min(nq, t * chunk), e = min(nq, b + chunk);
    int64_t s = 0;
    for (int64_t q = b; q < e; q++) s += cnt[q];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < CV_SCAN_T; off <<= 1) {
        const int64_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int64_t q = b; q < e; q++) {
        out_ptr[q] = run;
        run += cnt[q];
    }
    if (t == CV_SCAN_T - 1) out_ptr[nq] = part[t];
}

// One wave per query: the kept members in their order (before the run, after it).
__global__ __launch_bounds__(256) void cv_excl_copy_kernel(const int64_t* __restrict__ ptr,
                                                           const int32_t* __restrict__ idx, int64_t nq,
                                                           const int32_t* __restrict__ run_a,
                                                           const int32_t* __restrict__ run_b,
                                                           const int64_t* __restrict__ out_ptr,
                                                           int32_t* __restrict__ out_idx) {
    const int lane = threadIdx.x & 63;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += (int64_t)gridDim.x * 4) {
        const int64_t o = ptr[q], oo = out_ptr[q];
        const int n = (int)(ptr[q + 1] - o);
        const int a = run_a[q], b = run_b[q];
        for (int i = lane; i < a; i += 64) out_idx[oo + i] = idx[o + i];
        for (int i = b + lane; i < n; i += 64) out_idx[oo + a + (i - b)] = idx[o + i];
    }
}

// get_predicted_user_sim at every unknown index of every user (one thread per
// entry of the unknown-index CSR, entries unk_ptr[0] .. unk_ptr[nq]): pred[e]
// for entry e, NaN as x86 produces it.
__global__ __launch_bounds__(256) void cv_predict_kernel(const double* __restrict__ X,
                                                         const double* __restrict__ x_mean, int d,
                                                         const double* __restrict__ u_mean, int64_t nq,
                                                         const int64_t* __restrict__ unk_ptr,
                                                         const int32_t* __restrict__ unk_idx,
                                                         const int32_t* __restrict__ nb_idx,
                                                         const double* __restrict__ nb_sim,
                                                         const int32_t* __restrict__ nb_cnt, int P,
                                                         double* __restrict__ pred) {
    const int64_t e0 = unk_ptr[0], e1 = unk_ptr[nq];
    for (int64_t e = e0 + (int64_t)blockIdx.x * 256 + threadIdx.x; e < e1; e += (int64_t)gridDim.x * 256) {
        int64_t l = 0, h = nq;                  // the last q with unk_ptr[q] <= e (its list holds e)
        while (h - l > 1) {
            const int64_t mid = (l + h) >> 1;
            if (unk_ptr[mid] <= e) l = mid; else h = mid;
        }
        const int64_t q = l;
        const int index = unk_idx[e];
        if (index < 0 || index >= d) {          // not a dimension (the reference's at() throws): no prediction
            pred[e] = 0.0;
            continue;
        }
        double v = rc_predict_at(X, x_mean, d, nb_idx + q * P, nb_sim + q * P, nb_cnt[q], index, u_mean[q]);
        if (v != v) v = rc_predict_nan(X, x_mean, d, nb_idx + q * P, nb_sim + q * P, nb_cnt[q], index, u_mean[q]);
        pred[e] = v;
    }
}

__device__ inline double cv_rl(double v, int t) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), t);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), t);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// One fold's k_sum (main.cpp:419-424): k_sum = k_sum + fabs(old_score - pred)
// over the users that were calculated (hide_idx >= 0) and had neighbours, in
// fold order, and calc_user_num. One wave: the lanes load 64 errors, the adds
// go in order through readlane. err (may be NULL): the users' errors, -1.0
// for the skipped ones. A NaN k_sum is the positive quiet NaN (x86: fabs of the
// default NaN, propagated by every later add). carry: the chain continues from
// *k_sum_out / *cnt_out (a fold summed in chunks of users).
__global__ __launch_bounds__(64) void cv_fold_sum_kernel(int64_t F, const int32_t* __restrict__ hide_idx,
                                                         const double* __restrict__ old,
                                                         const double* __restrict__ pred,
                                                         const int64_t* __restrict__ nb_ptr, double* __restrict__ err,
                                                         double* __restrict__ k_sum_out, int64_t* __restrict__ cnt_out,
                                                         int carry) {
    const int lane = threadIdx.x;
    double k_sum = carry ? *k_sum_out : 0.0;
    int64_t calc = carry ? *cnt_out : 0;
    for (int64_t b = 0; b < F; b += 64) {
        const int64_t q = b + lane;
        bool c = false;
        double e = 0.0;
        if (q < F) {
            c = hide_idx[q] >= 0 && nb_ptr[q + 1] > nb_ptr[q];
            if (c) e = fabs(x86_nan(__dsub_rn(old[q], pred[q])));
            if (err) err[q] = c ? e : -1.0;
        }
        const unsigned long long mask = __ballot(c);
        const int n = (int)min<int64_t>(64, F - b);
        for (int t = 0; t < n; t++)
            if ((mask >> t) & 1ull) k_sum = __dadd_rn(k_sum, cv_rl(e, t));
        calc += __popcll(mask);
    }
    if (k_sum != k_sum) k_sum = __longlong_as_double(0x7FF8000000000000ll);
    if (lane == 0) {
        *k_sum_out = k_sum;
        *cnt_out = calc;
    }
}

int launch_cv_gather(hipStream_t s, const double* X, const double* x_mean, const int32_t* rows, int64_t M, int d,
                     double* W, double* w_mean) {
    if (M <= 0) return 0;
    hipLaunchKernelGGL(cv_gather_kernel, dim3(gsz(M * d, 256, 8192)), dim3(256), 0, s, X, x_mean, rows, M, d, W, w_mean);
    return kstatus("cv_gather_kernel");
}

int launch_cv_hide(hipStream_t s, const double* X, const double* x_mean, const int32_t* rows, int64_t M, int d,
                   const int64_t* unk_ptr, const int32_t* unk_idx, const int32_t* draw, double* H, double* h_mean,
                   int32_t* hide_idx, double* old) {
    if (M <= 0) return 0;
    hipLaunchKernelGGL(cv_hide_kernel, dim3(gsz(M, 256, 8192)), dim3(256), 0, s, X, x_mean, rows, M, d, unk_ptr, unk_idx,
                       draw, H, h_mean, hide_idx, old);
    return kstatus("cv_hide_kernel");
}

// cnt / run_a / run_b: [nq] scratch. out_ptr [nq + 1] always; out_idx (may be
// NULL: offsets only) must hold in_ptr[nq] rows at most.
int launch_cv_exclude(hipStream_t s, const int64_t* in_ptr, const int32_t* in_idx, int64_t nq, int32_t lo, int32_t hi,
                      int64_t* cnt, int32_t* run_a, int32_t* run_b, int64_t* out_ptr, int32_t* out_idx) {
    if (nq <= 0) {
        if (hipMemsetAsync(out_ptr, 0, 8, s) != hipSuccess) return kstatus("cv_exclude");
        return 0;
    }
    hipLaunchKernelGGL(cv_excl_count_kernel, dim3(gsz(nq, 256, 4096)), dim3(256), 0, s, in_ptr, in_idx, nq, lo, hi, cnt,
                       run_a, run_b);
    hipLaunchKernelGGL(cv_excl_scan_kernel, dim3(1), dim3(CV_SCAN_T), 0, s, cnt, nq, out_ptr);
    if (out_idx)
        hipLaunchKernelGGL(cv_excl_copy_kernel, dim3(gsz(nq, 4, 8192)), dim3(256), 0, s, in_ptr, in_idx, nq, run_a, run_b,
                           out_ptr, out_idx);
    return kstatus("cv_exclude");
}

int launch_cv_predict(hipStream_t s, const double* X, const double* x_mean, int d, const double* u_mean, int64_t nq,
                      int64_t entries, const int64_t* unk_ptr, const int32_t* unk_idx, const int32_t* nb_idx,
                      const double* nb_sim, const int32_t* nb_cnt, int P, double* pred) {
    if (nq <= 0 || entries <= 0) return 0;
    hipLaunchKernelGGL(cv_predict_kernel, dim3(gsz(entries, 256, 8192)), dim3(256), 0, s, X, x_mean, d, u_mean, nq,
                       unk_ptr, unk_idx, nb_idx, nb_sim, nb_cnt, P, pred);
    return kstatus("cv_predict_kernel");
}

int launch_cv_fold_sum(hipStream_t s, int64_t F, const int32_t* hide_idx, const double* old, const double* pred,
                       const int64_t* nb_ptr, double* err, double* k_sum_out, int64_t* cnt_out, bool carry) {
    hipLaunchKernelGGL(cv_fold_sum_kernel, dim3(1), dim3(64), 0, s, F, hide_idx, old, pred, nb_ptr, err, k_sum_out,
                       cnt_out, carry ? 1 : 0);
    return kstatus("cv_fold_sum_kernel");
}

}  // namespace lshkm
