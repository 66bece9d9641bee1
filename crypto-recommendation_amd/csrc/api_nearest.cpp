// api_nearest.cpp — C ABI of lshkm_min_vector_dist and its lists form
// (include/lshkm.h): min_vector_euclidean_dist / min_vector_cosine_dist
// (lib/utils.hpp:107-140) for nq queries at once. nearest_layout.h states the
// routing rule and every workspace; nearest.hip holds the kernels.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lshkm.h"
#include "common.h"
#include "index.h"
#include "kernels.h"
#include "nearest_layout.h"

using namespace lshkm;

template <typename T> static T* at(const Buf& b, size_t off) { return reinterpret_cast<T*>(b.as<char>() + off); }

// A failed call leaves nothing of its own running.
struct NearestSyncOnFail {
    hipStream_t s;
    const int* rc;
    ~NearestSyncOnFail() {
        if (*rc) (void)hipStreamSynchronize(s);
    }
};

static int nearest_args(lshkm_ctx ctx, Pts X, int64_t N, int d, Pts Q, int64_t nq, int metric, const double* dist) {
    LSHKM_CHECK(ctx && N >= 0 && N < (1ll << 31) && d >= 1 && nq >= 0 && nq < (1ll << 31) &&
                    (metric == LSHKM_METRIC_EUCLIDEAN || metric == LSHKM_METRIC_COSINE),
                LSHKM_ERR_ARG, "bad arguments (N < 2^31, d >= 1, metric euclidean or cosine)");
    LSHKM_CHECK(nq == 0 || (dist && Q.p && (X.p || N == 0)), LSHKM_ERR_ARG, "bad arguments (null pointer)");
    return 0;
}

static int nearest_finish(hipStream_t s, const char* who) {
    if (hipStreamSynchronize(s) != hipSuccess) {             // the workspace is reused by the next call
        set_error(std::string(who) + ": hipStreamSynchronize failed");
        return LSHKM_ERR_HIP;
    }
    return 0;
}

static int min_vector_dist(lshkm_ctx ctx, Pts X, int64_t N, int d, Pts Q, int64_t nq, int metric, double* dist,
                           int32_t* row) {
    int rc = 0;
    if ((rc = nearest_args(ctx, X, N, d, Q, nq, metric, dist))) return rc;
    if (nq == 0) return 0;
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unsigned long long* stats = (unsigned long long*)ctx->stats.p;
    const NearestSyncOnFail sync_guard{s, &rc};
    if (N == 0) {
        if ((rc = launch_nearest_empty(s, nq, dist, row))) return rc;
        return rc = nearest_finish(s, "lshkm_min_vector_dist");
    }
    const bool force_scan = test_switch("LSHKM_NEAREST_PATH", "exact");
    NearestRoute route = nearest_route(d, force_scan);
    Buf &bx = ctx->ws_nearest[0], &bq = ctx->ws_nearest[1], &bs = ctx->ws_nearest[2];
    const int dp = route == NearestRoute::screen ? nearest_dp(d) : 0;
    const NearestImage ix = nearest_image(N, dp), iq = nearest_image(nq, dp);
    if ((rc = bx.reserve(ix.bytes)) || (rc = bq.reserve(iq.bytes))) return rc;
    double *xn2 = at<double>(bx, ix.xa), *qn2 = at<double>(bq, iq.xa);
    if ((rc = launch_nearest_norms(s, X, N, d, metric, xn2)) || (rc = launch_nearest_norms(s, Q, nq, d, metric, qn2)))
        return rc;
    if (route == NearestRoute::screen) {
        int ncu = 0;
        if ((rc = device_cu_count(&ncu))) return rc;
        const NearestPlan plan = nearest_plan(N, nq, ncu, test_switch("LSHKM_NEAREST_CAP", "small"),
                                              test_switch("LSHKM_NEAREST_SEG", "small"));
        const NearestState st = nearest_state(nq, plan.cap);
        if ((rc = bs.reserve(st.bytes))) return rc;
        const NearestSide rows{at<float>(bx, ix.xh), at<float>(bx, ix.a), at<float>(bx, ix.rel), N};
        const NearestSide qs{at<float>(bq, iq.xh), at<float>(bq, iq.a), at<float>(bq, iq.rel), nq};
        const NearestKept kept{at<uint32_t>(bs, st.minkey), at<int32_t>(bs, st.cnt), at<int32_t>(bs, st.krow),
                               plan.seg_rows, plan.cap};
        unsigned int* counts = at<unsigned int>(bs, st.counts);
        int32_t* pois = at<int32_t>(bs, st.pois);
        if (hipMemsetAsync(counts, 0, 256, s) != hipSuccess) {
            set_error("lshkm_min_vector_dist: hipMemsetAsync failed");
            return rc = LSHKM_ERR_HIP;
        }
        if ((rc = launch_nearest_prep(s, X, N, d, dp, metric, rows, pois, counts + NEAREST_N_POISON)) ||
            (rc = launch_nearest_prep(s, Q, nq, d, dp, metric, qs, nullptr, nullptr)))
            return rc;
        unsigned int npois = 0;
        const D2H rd{&npois, counts + NEAREST_N_POISON, sizeof(npois)};
        if ((rc = d2h_batch(ctx, &rd, 1))) return rc;
        route = nearest_route_after_prep(npois);
        if (route == NearestRoute::screen) {
            int32_t* scan_list = at<int32_t>(bs, st.scan);
            if ((rc = launch_nearest_screen(s, dp, metric, rows, qs, kept, plan.tiles, plan.segs)) ||
                (rc = launch_nearest_collect(s, kept, qs.a, nq, scan_list, counts + NEAREST_N_SCAN, stats)) ||
                (rc = launch_nearest_settle(s, X, Q, nq, d, metric, nullptr, nullptr, kept, qs.a, pois,
                                            counts + NEAREST_N_POISON, xn2, qn2, dist, row, stats)) ||
                (rc = launch_nearest_scan(s, X, N, Q, nq, d, metric, scan_list, counts + NEAREST_N_SCAN, xn2, qn2, dist,
                                          row, stats)))
                return rc;
        }
    }
    if (route == NearestRoute::scan &&
        (rc = launch_nearest_scan(s, X, N, Q, nq, d, metric, nullptr, nullptr, xn2, qn2, dist, row, stats)))
        return rc;
    return rc = nearest_finish(s, "lshkm_min_vector_dist");
}

static int min_vector_dist_lists(lshkm_ctx ctx, Pts X, int64_t N, int d, Pts Q, int64_t nq, int metric,
                                 const int64_t* cand_ptr, const int32_t* cand_idx, double* dist, int32_t* row) {
    int rc = 0;
    if ((rc = nearest_args(ctx, X, N, d, Q, nq, metric, dist))) return rc;
    if (nq == 0) return 0;
    LSHKM_CHECK(cand_ptr, LSHKM_ERR_ARG, "bad arguments (null cand_ptr)");
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const NearestSyncOnFail sync_guard{s, &rc};
    int64_t total = 0;
    const D2H rt{&total, cand_ptr + nq, sizeof(total)};
    if ((rc = d2h_batch(ctx, &rt, 1))) return rc;
    LSHKM_CHECK(total >= 0 && (total == 0 || (cand_idx && X.p)), LSHKM_ERR_ARG, "bad candidate lists");
    Buf &bx = ctx->ws_nearest[0], &bq = ctx->ws_nearest[1], &bs = ctx->ws_nearest[2];
    const NearestState st = nearest_state(1, NEAREST_CAP_MIN);
    const NearestImage ix = nearest_image(N, 0), iq = nearest_image(nq, 0);
    if ((rc = bs.reserve(st.bytes)) || (rc = bx.reserve(ix.bytes)) || (rc = bq.reserve(iq.bytes))) return rc;
    double *xn2 = at<double>(bx, ix.xa), *qn2 = at<double>(bq, iq.xa);
    unsigned int *counts = at<unsigned int>(bs, st.counts), bad = 0;
    if (hipMemsetAsync(counts, 0, 256, s) != hipSuccess) {
        set_error("lshkm_min_vector_dist_lists: hipMemsetAsync failed");
        return rc = LSHKM_ERR_HIP;
    }
    const D2H rb{&bad, counts + NEAREST_N_BADIDX, sizeof(bad)};
    if ((rc = launch_nearest_check(s, cand_ptr, nq, cand_idx, total, N, counts + NEAREST_N_BADIDX)) ||
        (rc = d2h_batch(ctx, &rb, 1)))
        return rc;
    if (bad) {
        set_error("bad candidate lists (cand_ptr must start at 0 and not decrease; indexes in [0, N))");
        return rc = LSHKM_ERR_ARG;
    }
    if ((rc = launch_nearest_norms(s, X, total ? N : 0, d, metric, xn2)) ||
        (rc = launch_nearest_norms(s, Q, nq, d, metric, qn2)) ||
        (rc = launch_nearest_settle(s, X, Q, nq, d, metric, cand_ptr, cand_idx, NearestKept{}, nullptr, nullptr, nullptr,
                                    xn2, qn2, dist, row, (unsigned long long*)ctx->stats.p)))
        return rc;
    return rc = nearest_finish(s, "lshkm_min_vector_dist_lists");
}

extern "C" {

int lshkm_min_vector_dist(lshkm_ctx ctx, const float* X, int64_t N, int d, const float* Q, int64_t nq, int metric,
                          double* dist, int32_t* row) {
    return min_vector_dist(ctx, Pts(X), N, d, Pts(Q), nq, metric, dist, row);
}
int lshkm_min_vector_dist_f64(lshkm_ctx ctx, const double* X, int64_t N, int d, const double* Q, int64_t nq, int metric,
                              double* dist, int32_t* row) {
    return min_vector_dist(ctx, Pts(X), N, d, Pts(Q), nq, metric, dist, row);
}
int lshkm_min_vector_dist_lists(lshkm_ctx ctx, const float* X, int64_t N, int d, const float* Q, int64_t nq, int metric,
                                const int64_t* cand_ptr, const int32_t* cand_idx, double* dist, int32_t* row) {
    return min_vector_dist_lists(ctx, Pts(X), N, d, Pts(Q), nq, metric, cand_ptr, cand_idx, dist, row);
}
int lshkm_min_vector_dist_lists_f64(lshkm_ctx ctx, const double* X, int64_t N, int d, const double* Q, int64_t nq,
                                    int metric, const int64_t* cand_ptr, const int32_t* cand_idx, double* dist,
                                    int32_t* row) {
    return min_vector_dist_lists(ctx, Pts(X), N, d, Pts(Q), nq, metric, cand_ptr, cand_idx, dist, row);
}

}  // extern "C"
