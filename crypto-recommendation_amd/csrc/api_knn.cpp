// api_knn.cpp — C ABI of lshkm_knn and its lists form (include/lshkm.h): the k
// exact nearest rows of every query. knn_layout.h states the routing rule and
// the workspace; knn.hip holds the kernels; the f32 images, the prep, the norms
// and the lists check are lshkm_min_vector_dist's (nearest.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lshkm.h"
#include "common.h"
#include "index.h"
#include "kernels.h"
#include "knn_layout.h"

using namespace lshkm;

static_assert(KNN_KMAX == LSHKM_KNN_KMAX, "knn_layout.h and lshkm.h state one limit");

template <typename T> static T* at(const Buf& b, size_t off) { return reinterpret_cast<T*>(b.as<char>() + off); }

// A failed call leaves nothing of its own running.
struct KnnSyncOnFail {
    hipStream_t s;
    const int* rc;
    ~KnnSyncOnFail() {
        if (*rc) (void)hipStreamSynchronize(s);
    }
};

static int knn_args(lshkm_ctx ctx, Pts X, int64_t N, int d, Pts Q, int64_t nq, int metric, int k, const int32_t* row,
                    const double* dist) {
    LSHKM_CHECK(ctx && N >= 0 && N < (1ll << 31) && d >= 1 && nq >= 0 && nq < (1ll << 31) &&
                    (metric == LSHKM_METRIC_EUCLIDEAN || metric == LSHKM_METRIC_COSINE),
                LSHKM_ERR_ARG, "bad arguments (N < 2^31, d >= 1, metric euclidean or cosine)");
    LSHKM_CHECK(k >= 1 && k <= LSHKM_KNN_KMAX, LSHKM_ERR_ARG, "bad arguments (1 <= k <= LSHKM_KNN_KMAX)");
    LSHKM_CHECK(nq == 0 || (row && dist && Q.p && (X.p || N == 0)), LSHKM_ERR_ARG, "bad arguments (null pointer)");
    return 0;
}

static int knn_finish(hipStream_t s, const char* who) {
    if (hipStreamSynchronize(s) != hipSuccess) {             // the workspace is reused by the next call
        set_error(std::string(who) + ": hipStreamSynchronize failed");
        return LSHKM_ERR_HIP;
    }
    return 0;
}

static int knn(lshkm_ctx ctx, Pts X, int64_t N, int d, Pts Q, int64_t nq, int metric, int k, int32_t* row, double* dist,
               int32_t* cnt) {
    int rc = 0;
    if ((rc = knn_args(ctx, X, N, d, Q, nq, metric, k, row, dist))) return rc;
    if (nq == 0) return 0;
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unsigned long long* stats = (unsigned long long*)ctx->stats.p;
    const KnnSyncOnFail sync_guard{s, &rc};
    if (N == 0) {
        if ((rc = launch_knn_empty(s, nq, k, row, dist, cnt))) return rc;
        return rc = knn_finish(s, "lshkm_knn");
    }
    int ncu = 0;
    if ((rc = device_cu_count(&ncu))) return rc;
    const KnnPlan plan =
        knn_plan(N, nq, k, ncu, test_switch("LSHKM_KNN_CAP", "small"), test_switch("LSHKM_KNN_SEG", "small"));
    KnnRoute route = knn_route(d, k, plan.groups, test_switch("LSHKM_KNN_PATH", "exact"));
    Buf &bx = ctx->ws_nearest[0], &bq = ctx->ws_nearest[1], &bs = ctx->ws_knn;
    const int dp = route == KnnRoute::screen ? nearest_dp(d) : 0;
    const NearestImage ix = nearest_image(N, dp), iq = nearest_image(nq, dp);
    if ((rc = bx.reserve(ix.bytes)) || (rc = bq.reserve(iq.bytes))) return rc;
    double *xn2 = at<double>(bx, ix.xa), *qn2 = at<double>(bq, iq.xa);
    if ((rc = launch_nearest_norms(s, X, N, d, metric, xn2)) || (rc = launch_nearest_norms(s, Q, nq, d, metric, qn2)))
        return rc;
    if (route == KnnRoute::screen) {
        const KnnState st = knn_state(nq, plan.groups, plan.cap);
        if ((rc = bs.reserve(st.bytes))) return rc;
        const NearestSide rows{at<float>(bx, ix.xh), at<float>(bx, ix.a), at<float>(bx, ix.rel), N};
        const NearestSide qs{at<float>(bq, iq.xh), at<float>(bq, iq.a), at<float>(bq, iq.rel), nq};
        const KnnKept kept{at<uint32_t>(bs, st.gkey), at<uint32_t>(bs, st.tau), at<int32_t>(bs, st.cnt),
                           at<int32_t>(bs, st.krow), plan.seg_rows, plan.groups, plan.grp_shift, plan.cap, k};
        unsigned int* counts = at<unsigned int>(bs, st.counts);
        int32_t* pois = at<int32_t>(bs, st.pois);
        if (hipMemsetAsync(counts, 0, 256, s) != hipSuccess) {
            set_error("lshkm_knn: hipMemsetAsync failed");
            return rc = LSHKM_ERR_HIP;
        }
        if ((rc = launch_nearest_prep(s, X, N, d, dp, metric, rows, pois, counts + NEAREST_N_POISON)) ||
            (rc = launch_nearest_prep(s, Q, nq, d, dp, metric, qs, nullptr, nullptr)))
            return rc;
        unsigned int npois = 0;
        const D2H rd{&npois, counts + NEAREST_N_POISON, sizeof(npois)};
        if ((rc = d2h_batch(ctx, &rd, 1))) return rc;
        route = knn_route_after_prep(N, k, npois);
        if (route == KnnRoute::screen) {
            int32_t* scan_list = at<int32_t>(bs, st.scan);
            if ((rc = launch_knn_screen(s, dp, metric, rows, qs, kept, plan.tiles, plan.segs)) ||
                (rc = launch_knn_collect(s, kept, qs.a, nq, scan_list, counts + NEAREST_N_SCAN, stats)) ||
                (rc = launch_knn_settle(s, X, Q, nq, d, metric, k, nullptr, nullptr, kept, qs.a, pois,
                                        counts + NEAREST_N_POISON, xn2, qn2, row, dist, cnt, stats)) ||
                (rc = launch_knn_scan(s, X, N, Q, nq, d, metric, k, scan_list, counts + NEAREST_N_SCAN, xn2, qn2, row,
                                      dist, cnt, stats)))
                return rc;
        }
    }
    if (route == KnnRoute::scan &&
        (rc = launch_knn_scan(s, X, N, Q, nq, d, metric, k, nullptr, nullptr, xn2, qn2, row, dist, cnt, stats)))
        return rc;
    return rc = knn_finish(s, "lshkm_knn");
}

static int knn_lists(lshkm_ctx ctx, Pts X, int64_t N, int d, Pts Q, int64_t nq, int metric, int k,
                     const int64_t* cand_ptr, const int32_t* cand_idx, int32_t* row, double* dist, int32_t* cnt) {
    int rc = 0;
    if ((rc = knn_args(ctx, X, N, d, Q, nq, metric, k, row, dist))) return rc;
    if (nq == 0) return 0;
    LSHKM_CHECK(cand_ptr, LSHKM_ERR_ARG, "bad arguments (null cand_ptr)");
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const KnnSyncOnFail sync_guard{s, &rc};
    int64_t total = 0;
    const D2H rt{&total, cand_ptr + nq, sizeof(total)};
    if ((rc = d2h_batch(ctx, &rt, 1))) return rc;
    LSHKM_CHECK(total >= 0 && (total == 0 || (cand_idx && X.p)), LSHKM_ERR_ARG, "bad candidate lists");
    Buf &bx = ctx->ws_nearest[0], &bq = ctx->ws_nearest[1], &bs = ctx->ws_knn;
    const KnnState st = knn_state(1, 1, 1);
    const NearestImage ix = nearest_image(N, 0), iq = nearest_image(nq, 0);
    if ((rc = bs.reserve(st.bytes)) || (rc = bx.reserve(ix.bytes)) || (rc = bq.reserve(iq.bytes))) return rc;
    double *xn2 = at<double>(bx, ix.xa), *qn2 = at<double>(bq, iq.xa);
    unsigned int *counts = at<unsigned int>(bs, st.counts), bad = 0;
    if (hipMemsetAsync(counts, 0, 256, s) != hipSuccess) {
        set_error("lshkm_knn_lists: hipMemsetAsync failed");
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
        (rc = launch_knn_settle(s, X, Q, nq, d, metric, k, cand_ptr, cand_idx, KnnKept{}, nullptr, nullptr, nullptr, xn2,
                                qn2, row, dist, cnt, (unsigned long long*)ctx->stats.p)))
        return rc;
    return rc = knn_finish(s, "lshkm_knn_lists");
}

extern "C" {

int lshkm_knn(lshkm_ctx ctx, const float* X, int64_t N, int d, const float* Q, int64_t nq, int metric, int k,
              int32_t* row, double* dist, int32_t* cnt) {
    return knn(ctx, Pts(X), N, d, Pts(Q), nq, metric, k, row, dist, cnt);
}
int lshkm_knn_f64(lshkm_ctx ctx, const double* X, int64_t N, int d, const double* Q, int64_t nq, int metric, int k,
                  int32_t* row, double* dist, int32_t* cnt) {
    return knn(ctx, Pts(X), N, d, Pts(Q), nq, metric, k, row, dist, cnt);
}
int lshkm_knn_lists(lshkm_ctx ctx, const float* X, int64_t N, int d, const float* Q, int64_t nq, int metric, int k,
                    const int64_t* cand_ptr, const int32_t* cand_idx, int32_t* row, double* dist, int32_t* cnt) {
    return knn_lists(ctx, Pts(X), N, d, Pts(Q), nq, metric, k, cand_ptr, cand_idx, row, dist, cnt);
}
int lshkm_knn_lists_f64(lshkm_ctx ctx, const double* X, int64_t N, int d, const double* Q, int64_t nq, int metric, int k,
                        const int64_t* cand_ptr, const int32_t* cand_idx, int32_t* row, double* dist, int32_t* cnt) {
    return knn_lists(ctx, Pts(X), N, d, Pts(Q), nq, metric, k, cand_ptr, cand_idx, row, dist, cnt);
}

}  // extern "C"
