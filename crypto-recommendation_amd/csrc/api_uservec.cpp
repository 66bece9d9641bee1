// api_uservec.cpp — C ABI of the user vectors from scored tweets
// (include/lshkm.h): the update loop and the finishing loop of
// tweets_to_user_vectors / clusters_to_user_vectors (lib/crypto_rec.hpp:78-210).
// uservec.hip holds the kernels; the workspace is ctx->ws_call (both entry
// points drain the stream before they return).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/lshkm.h"
#include "common.h"
#include "index.h"
#include "kernels.h"

using namespace lshkm;

namespace {

int read_back(lshkm_ctx ctx, const void* dev, void* host, size_t bytes) {
    const D2H r{host, dev, bytes};
    return d2h_batch(ctx, &r, 1);
}

int user_sums(lshkm_ctx ctx, const UvVisits& q, const double* carry_sum, const uint8_t* carry_known, double* sum,
              uint8_t* known) {
    hipStream_t s = ctx->stream;
    const int64_t nkeys = q.G * q.C;
    Buf &cnt = ctx->ws_call[0], &off = ctx->ws_call[1], &scan = ctx->ws_call[2], &pairs = ctx->ws_call[3],
        &sortws = ctx->ws_call[4], &rowp = ctx->ws_call[5], &lng = ctx->ws_call[6], &words = ctx->ws_call[7];
    int rc;
    if ((rc = words.reserve(64)) || (rc = cnt.reserve(8 * (size_t)std::max<int64_t>(q.V, 1))) ||
        (rc = off.reserve(8 * (size_t)(q.V + 1))) || (rc = scan.reserve(scan_ws_bytes(q.V))))
        return rc;
    uint32_t* flag = words.as<uint32_t>();          // [0]: the checks' flag, [1]: the long chains' count
    LSHKM_HIP(hipMemsetAsync(flag, 0, 8, s));
    // the range checks, on the device, before anything is written
    uint32_t bad = 0;
    if ((rc = launch_uv_check(s, q, false, flag)) || (rc = read_back(ctx, flag, &bad, 4))) return rc;
    if (!bad && q.T > 0 && ((rc = launch_uv_check(s, q, true, flag)) || (rc = read_back(ctx, flag, &bad, 4)))) return rc;
    LSHKM_CHECK(!(bad & 1u), LSHKM_ERR_ARG, "tw holds a tweet number outside [-1, T)");
    LSHKM_CHECK(!(bad & 2u), LSHKM_ERR_ARG, "grp holds a group outside [-1, G)");
    LSHKM_CHECK(!(bad & 8u), LSHKM_ERR_ARG, "bad coin lists (ci_ptr must start at 0 and not decrease)");
    LSHKM_CHECK(!(bad & 4u), LSHKM_ERR_ARG, "ci_idx holds a coin index outside [0, C)");
    if (nkeys == 0) return 0;
    int64_t E = 0;
    if (q.V > 0) {
        if ((rc = launch_uv_count(s, q, cnt.as<int64_t>())) ||
            (rc = launch_scan_i64(s, cnt.as<int64_t>(), q.V, off.as<int64_t>(), scan.as<int64_t>())) ||
            (rc = read_back(ctx, off.as<int64_t>() + q.V, &E, 8)))
            return rc;
    }
    LSHKM_CHECK(E < ((int64_t)1 << 31), LSHKM_ERR_UNSUPPORTED, "2^31 (tweet, coin) incidences or more in one call");
    const size_t En = (size_t)std::max<int64_t>(E, 1);
    if ((rc = pairs.reserve(4 * 4 * En)) || (rc = sortws.reserve(uv_sort_bytes(E, nkeys))) ||
        (rc = rowp.reserve(8 * (size_t)(nkeys + 1))) || (rc = lng.reserve(4 * (size_t)nkeys)))
        return rc;
    int32_t* keys = pairs.as<int32_t>();
    return launch_uv_sums(s, q, off.as<int64_t>(), E, carry_sum, carry_known, keys, keys + En, keys + 2 * En,
                          keys + 3 * En, sortws.p, rowp.as<int64_t>(), lng.as<int32_t>(), flag + 1, sum, known);
}

}  // namespace

extern "C" {

int lshkm_user_sums(lshkm_ctx ctx, const int32_t* tw, const int32_t* grp, int64_t V, const double* score,
                    const int64_t* ci_ptr, const int32_t* ci_idx, int64_t T, int64_t G, int C, const double* carry_sum,
                    const uint8_t* carry_known, double* sum, uint8_t* known) {
    LSHKM_CHECK(ctx && V >= 0 && T >= 0 && G >= 0 && C >= 0, LSHKM_ERR_ARG, "bad arguments");
    LSHKM_CHECK((V == 0 || (tw && grp)) && (T == 0 || (score && ci_ptr)) && (G * (int64_t)C == 0 || (sum && known)),
                LSHKM_ERR_ARG, "a NULL array");
    LSHKM_CHECK(!carry_sum == !carry_known, LSHKM_ERR_ARG, "the carry is both arrays or neither");
    LSHKM_CHECK(G < ((int64_t)1 << 31) && G * (int64_t)C < ((int64_t)1 << 31), LSHKM_ERR_UNSUPPORTED,
                "G * C of 2^31 or more");
    LSHKM_CHECK(V < ((int64_t)1 << 31) && T < ((int64_t)1 << 31), LSHKM_ERR_UNSUPPORTED, "2^31 visits or tweets or more");
    LSHKM_HIP(hipSetDevice(ctx->device));
    const UvVisits q{tw, grp, V, score, ci_ptr, ci_idx, T, G, C};
    const int rc = user_sums(ctx, q, carry_sum, carry_known, sum, known);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is reused by the next call
    return 0;
}

int lshkm_user_finish(lshkm_ctx ctx, const double* sum, const uint8_t* known, int64_t G, int C, double* U, double* mean,
                      int64_t* unk_ptr, int32_t* unk_idx, int32_t* src, int64_t* n_kept_host) {
    LSHKM_CHECK(ctx && G >= 0 && C >= 0 && unk_ptr && n_kept_host, LSHKM_ERR_ARG, "bad arguments");
    LSHKM_CHECK(G == 0 || (mean && src && (C == 0 || (sum && known && U && unk_idx))), LSHKM_ERR_ARG, "a NULL array");
    LSHKM_CHECK(G < ((int64_t)1 << 31) && G * (int64_t)C < ((int64_t)1 << 31), LSHKM_ERR_UNSUPPORTED,
                "G * C of 2^31 or more");
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    *n_kept_host = 0;
    if (G == 0) {
        LSHKM_HIP(hipMemsetAsync(unk_ptr, 0, 8, s));
        LSHKM_HIP(hipStreamSynchronize(s));
        return 0;
    }
    Buf &cnts = ctx->ws_call[0], &offs = ctx->ws_call[1], &scan = ctx->ws_call[2], &mn = ctx->ws_call[3];
    int rc;
    if ((rc = cnts.reserve(2 * 8 * (size_t)G)) || (rc = offs.reserve(2 * 8 * (size_t)(G + 1))) ||
        (rc = scan.reserve(scan_ws_bytes(G))) || (rc = mn.reserve(8 * (size_t)G)))
        return rc;
    int64_t* row_off = offs.as<int64_t>();
    if ((rc = launch_uv_finish(s, sum, known, G, C, cnts.as<int64_t>(), cnts.as<int64_t>() + G, row_off,
                               row_off + G + 1, mn.as<double>(), scan.as<int64_t>(), U, mean, unk_ptr, unk_idx, src)) ||
        (rc = read_back(ctx, row_off + G, n_kept_host, 8))) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    return 0;
}

}  // extern "C"
