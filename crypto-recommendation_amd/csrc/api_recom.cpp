// api_recom.cpp — C ABI of the recommend step (include/lshkm.h): batched
// get_P_closest and get_top_N_recom (lib/crypto_rec.hpp:213-325).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/lshkm.h"
#include "common.h"
#include "index.h"
#include "kernels.h"
#include "lshpc_layout.h"

using namespace lshkm;

static int read_i64(lshkm_ctx ctx, const int64_t* dev, int64_t* host) {
    const D2H r{host, dev, sizeof(int64_t)};
    return d2h_batch(ctx, &r, 1);
}

// Host vectors handed to hipMemcpyAsync must outlive the copy: declared after
// them, this waits for the stream on every exit path (its destructor runs
// before theirs); with only_if, on the exit paths that left *only_if nonzero
// (a failed call leaves nothing of its own running).
struct StreamSyncOnExit {
    hipStream_t s;
    const int* only_if = nullptr;
    ~StreamSyncOnExit() {
        if (!only_if || *only_if) (void)hipStreamSynchronize(s);
    }
};

// get_P_closest's launches for candidate lists of `total` rows (at least the
// lists' real total), on the stream, in the ws_call workspace; no host wait.
static int p_closest_launch(lshkm_ctx ctx, const double* X, int64_t N, int d, const double* U, int64_t nq,
                            const int64_t* cand_ptr, const int32_t* cand_idx, int64_t total, int P, int32_t* out_idx,
                            double* out_sim, int32_t* out_cnt) {
    Buf &xa = ctx->ws_call[0], &sim = ctx->ws_call[1], &key = ctx->ws_call[2], &pos = ctx->ws_call[3],
        &replay = ctx->ws_call[4], &count = ctx->ws_call[5];
    const size_t T = (size_t)(total > 0 ? total : 1);
    int rc;
    if ((rc = xa.reserve(sizeof(double) * N)) || (rc = sim.reserve(sizeof(double) * T)) ||
        (rc = key.reserve(sizeof(double) * T)) || (rc = pos.reserve(sizeof(int32_t) * T)) ||
        (rc = replay.reserve(sizeof(int32_t) * nq)) || (rc = count.reserve(sizeof(unsigned int))))
        return rc;
    if ((rc = launch_rc_norms(ctx->stream, X, N, d, xa.as<double>()))) return rc;
    return launch_rc_p_closest(ctx->stream, X, xa.as<double>(), d, U, nq, cand_ptr, cand_idx, P, sim.as<double>(),
                               key.as<double>(), pos.as<int32_t>(), out_idx, out_sim, out_cnt, replay.as<int32_t>(),
                               count.as<unsigned int>());
}

extern "C" {

int lshkm_p_closest(lshkm_ctx ctx, const double* X, int64_t N, int d, const double* U, int64_t nq,
                    const int64_t* cand_ptr, const int32_t* cand_idx, int P, int32_t* out_idx, double* out_sim,
                    int32_t* out_cnt) {
    LSHKM_CHECK(ctx && X && U && cand_ptr && out_idx && out_sim && out_cnt && N >= 1 && d >= 1 && nq >= 0 && P >= 1,
                LSHKM_ERR_ARG, "bad arguments");
    if (nq == 0) return 0;
    LSHKM_HIP(hipSetDevice(ctx->device));
    int64_t total = 0;
    int rc;
    if ((rc = read_i64(ctx, cand_ptr + nq, &total))) return rc;
    LSHKM_CHECK(total >= 0 && (total == 0 || cand_idx), LSHKM_ERR_ARG, "bad candidate lists");
    if ((rc = p_closest_launch(ctx, X, N, d, U, nq, cand_ptr, cand_idx, total, P, out_idx, out_sim, out_cnt))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is reused by the next call
    return 0;
}

int lshkm_top_n_recom(lshkm_ctx ctx, const double* X, const double* x_mean, int64_t N, int d, const double* u_mean,
                      int64_t nq, const int64_t* unk_ptr, const int32_t* unk_idx, const int32_t* nb_idx,
                      const double* nb_sim, const int32_t* nb_cnt, int P, int n_top, int32_t* out) {
    LSHKM_CHECK(ctx && X && x_mean && u_mean && unk_ptr && nb_idx && nb_sim && nb_cnt && out && N >= 1 && d >= 1 &&
                    nq >= 0 && P >= 1 && n_top >= 0,
                LSHKM_ERR_ARG, "bad arguments");
    if (nq == 0 || n_top == 0) return 0;
    LSHKM_HIP(hipSetDevice(ctx->device));
    int64_t total = 0;
    int rc;
    if ((rc = read_i64(ctx, unk_ptr + nq, &total))) return rc;
    LSHKM_CHECK(total >= 0 && (total == 0 || unk_idx), LSHKM_ERR_ARG, "bad unknown-index lists");
    Buf &pred = ctx->ws_call[0], &pidx = ctx->ws_call[1];
    const size_t M = (size_t)(total > 0 ? total : 1);
    if ((rc = pred.reserve(sizeof(double) * M)) || (rc = pidx.reserve(sizeof(int32_t) * M))) return rc;
    if ((rc = launch_rc_top_n(ctx->stream, X, x_mean, d, u_mean, nq, unk_ptr, unk_idx, nb_idx, nb_sim, nb_cnt, P, n_top,
                              pred.as<double>(), pidx.as<int32_t>(), out))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"

template <typename T> static T* at(const Buf& b, size_t off) { return reinterpret_cast<T*>(b.as<char>() + off); }

// ------------------------------------ LSH recommender: P closest from the index
// lshkm_lsh_p_closest. lshpc_layout.h states the routing rule and every
// workspace; lsh_closest.hip is the screen.
//
// The lists path: lshkm_lsh_query_f64(filtered) -> the exclusion ->
// get_P_closest on the users of `list` (ascending), gathered, in chunks whose
// candidate lists fit cand_cap rows; the results scattered to the users' slots.
static int lshpc_lists(lshkm_lsh lsh, const double* X, const double* U, const std::vector<int32_t>& list,
                       int32_t excl_lo, int32_t excl_hi, int P, int64_t cand_cap, int32_t* out_idx, double* out_sim,
                       int32_t* out_cnt, int64_t* ncand) {
    lshkm_ctx ctx = lsh->ctx;
    hipStream_t s = ctx->stream;
    const int64_t m_all = (int64_t)list.size(), N = lsh->N;
    const int d = lsh->proj.d, L = lsh->proj.L, k = lsh->proj.k;
    if (m_all == 0) return 0;
    // first guess from the mean bucket load, as lshkm_lsh_validate10's; a chunk
    // whose lists come out larger is cut down below
    const int64_t buckets = lsh->metric == LSHKM_METRIC_EUCLIDEAN ? std::max<int64_t>(lsh->nb, 1)
                                                                  : (int64_t)1 << std::min(k, 40);
    int64_t chunk = std::max<int64_t>(
        1, std::min<int64_t>(m_all, cand_cap / std::max<int64_t>(1, (int64_t)L * (N / buckets + 1))));
    Buf &bu = ctx->ws_lshpc[4], &bq = ctx->ws_lshpc[5], &be = ctx->ws_lshpc[6];
    int rc;
    for (int64_t i0 = 0; i0 < m_all;) {
        const int64_t n = std::min(m_all - i0, chunk);
        // Ug | qptr | eptr | scr (int64) | gsim | list | ra | rb | gcnt | gidx
        const size_t oUg = 0, oq = oUg + lshpc_round256(8 * (size_t)n * d), oe = oq + lshpc_round256(8 * (size_t)(n + 1)),
                     osc = oe + lshpc_round256(8 * (size_t)(n + 1)), ogs = osc + lshpc_round256(8 * (size_t)n),
                     oli = ogs + lshpc_round256(8 * (size_t)n * P), ora = oli + lshpc_round256(4 * (size_t)n),
                     orb = ora + lshpc_round256(4 * (size_t)n), ogc = orb + lshpc_round256(4 * (size_t)n),
                     ogi = ogc + lshpc_round256(4 * (size_t)n), bytes = ogi + lshpc_round256(4 * (size_t)n * P);
        if ((rc = bu.reserve(bytes))) return rc;
        double* Ug = at<double>(bu, oUg);
        int64_t *qptr = at<int64_t>(bu, oq), *eptr = at<int64_t>(bu, oe);
        int32_t* dlist = at<int32_t>(bu, oli);
        const H2D up{dlist, list.data() + i0, 4 * (size_t)n};
        if ((rc = h2d_batch(ctx, &up, 1)) || (rc = launch_lshpc_gather(s, U, d, dlist, n, Ug))) return rc;
        int64_t total = 0;
        if ((rc = lshkm_lsh_query_f64(lsh, Ug, n, nullptr, 1, qptr, nullptr, 0, &total))) return rc;
        if (total > cand_cap && n > 1) {                 // size the chunk by this one's lists and ask again
            chunk = std::max<int64_t>(1, (int64_t)((double)n * (double)cand_cap / (double)total));
            continue;
        }
        const size_t T = (size_t)std::max<int64_t>(total, 1);
        if ((rc = bq.reserve(4 * T)) || (rc = be.reserve(4 * T))) return rc;
        if ((rc = lshkm_lsh_query_f64(lsh, Ug, n, nullptr, 1, qptr, bq.as<int32_t>(), total, &total))) return rc;
        if ((rc = launch_cv_exclude(s, qptr, bq.as<int32_t>(), n, excl_lo, excl_hi, at<int64_t>(bu, osc),
                                    at<int32_t>(bu, ora), at<int32_t>(bu, orb), eptr, be.as<int32_t>())))
            return rc;
        if ((rc = p_closest_launch(ctx, X, N, d, Ug, n, eptr, be.as<int32_t>(), total, P, at<int32_t>(bu, ogi),
                                   at<double>(bu, ogs), at<int32_t>(bu, ogc))))
            return rc;
        if ((rc = launch_lshpc_scatter(s, dlist, n, P, at<int32_t>(bu, ogi), at<double>(bu, ogs), at<int32_t>(bu, ogc),
                                       eptr, out_idx, out_sim, out_cnt, ncand)))
            return rc;
        i0 += n;
    }
    return 0;
}

// The screen over every user of a call, for both entry points. row_code
// [N][L]: the rows' bucket IDs of k bits each (a cube: L = 1, the vertices);
// probe: the cube's candidacy (NULL: the LSH tables').
struct ScreenJob {
    const double *X, *U;
    int64_t N, nq;
    int d, L, k, P;
    const int32_t* row_code;
    int32_t excl_lo, excl_hi;
    const CubeProbe* probe;
};

// One pass over X and one over U (the reference's sums of squares, the users'
// codes through user_codes(out [nq][L]), the f32 images), then the users in
// chunks (lshpc_plan): the screen, the join, the exact top-(P+1) over the kept
// rows, the collect. handed <- the users handed back, ascending; *ucode <- the
// users' codes on the device (ws_lshpc[1]).
template <typename UserCodes>
static int lshpc_screen_all(lshkm_ctx ctx, const ScreenJob& j, UserCodes user_codes, bool small_cap, int32_t* out_idx,
                            double* out_sim, int32_t* out_cnt, int64_t* ncand, std::vector<int32_t>& handed,
                            const int32_t** ucode) {
    hipStream_t s = ctx->stream;
    unsigned long long* stats = (unsigned long long*)ctx->stats.p;
    const int64_t N = j.N, nq = j.nq;
    const int d = j.d, L = j.L, k = j.k, P = j.P;
    int rc, ncu = 0;
    if ((rc = device_cu_count(&ncu))) return rc;
    const size_t budget = test_switch("LSHKM_LSHPC_BUDGET", "small") ? (size_t)1 << 20 : LSHPC_BUDGET;
    const LshpcPlan plan = lshpc_plan(N, nq, P, ncu, small_cap, budget);
    const int dp = lshpc_dp(d);
    const LshpcImage ix = lshpc_image(N, dp, 0), iu = lshpc_image(nq, dp, L);
    const LshpcChunk cmax = lshpc_chunk(plan.chunk, plan.cap, plan.segs);
    Buf &bx = ctx->ws_lshpc[0], &bu = ctx->ws_lshpc[1], &bc = ctx->ws_lshpc[2], &bh = ctx->ws_lshpc[3];
    if ((rc = bx.reserve(ix.bytes)) || (rc = bu.reserve(iu.bytes)) || (rc = bc.reserve(cmax.bytes)) ||
        (rc = bh.reserve(256 + 4 * (size_t)nq)))
        return rc;
    const LshpcSide rows{at<float>(bx, ix.xh), at<uint32_t>(bx, ix.code), at<float>(bx, ix.inv), at<float>(bx, ix.rel),
                         N};
    const LshpcSide users{at<float>(bu, iu.xh), at<uint32_t>(bu, iu.code), at<float>(bu, iu.inv),
                          at<float>(bu, iu.rel), nq};
    double* xa = at<double>(bx, ix.xa);
    int32_t* ubucket = at<int32_t>(bu, iu.bucket);
    *ucode = ubucket;
    unsigned int* handed_count = bh.as<unsigned int>();
    int32_t* handed_dev = at<int32_t>(bh, 256);
    if ((rc = launch_rc_norms(s, j.X, N, d, xa)) || (rc = launch_lshpc_prep(s, j.X, N, d, dp, xa, j.row_code, L, k, rows)) ||
        (rc = user_codes(ubucket)) || (rc = launch_rc_norms(s, j.U, nq, d, at<double>(bu, iu.xa))) ||
        (rc = launch_lshpc_prep(s, j.U, nq, d, dp, at<double>(bu, iu.xa), ubucket, L, k, users)))
        return rc;
    if (hipMemsetAsync(handed_count, 0, sizeof(unsigned int), s) != hipSuccess) {
        set_error("lshpc screen: hipMemsetAsync failed");
        return LSHKM_ERR_HIP;
    }
    for (int64_t u0 = 0; u0 < nq; u0 += plan.chunk) {
        const int64_t n = std::min(plan.chunk, nq - u0);
        const LshpcChunk c = lshpc_chunk(n, plan.cap, plan.segs);
        const LshpcKept kept{at<float>(bc, c.klo), at<float>(bc, c.khi), at<int32_t>(bc, c.krow),
                             at<int32_t>(bc, c.state), c.np, plan.seg_rows, plan.cap, plan.segs};
        const LshpcSide chunk_users{users.xh + (size_t)u0 * dp, users.code + u0, users.inv + u0, users.rel + u0, n};
        unsigned int* replay_count = at<unsigned int>(bc, c.counts);
        if ((rc = j.probe ? launch_cubepc_screen(s, dp, rows, chunk_users, P, *j.probe, kept)
                          : launch_lshpc_screen(s, dp, rows, chunk_users, j.excl_lo, j.excl_hi, P, L, k, kept)) ||
            (rc = launch_lshpc_join(s, kept, n, P, at<int64_t>(bc, c.nkept), ncand ? ncand + u0 : nullptr,
                                    at<int64_t>(bc, c.cptr), at<int32_t>(bc, c.cidx), stats)) ||
            // the exact top-(P+1) over the kept rows; its replay list (a NaN,
            // or a tie in the first P+1) is returned, not replayed: Lomuto's
            // order depends on the whole list, which only the lists path has
            (rc = launch_rc_p_closest(s, j.X, xa, d, j.U + (size_t)u0 * d, n, at<int64_t>(bc, c.cptr),
                                      at<int32_t>(bc, c.cidx), P, at<double>(bc, c.sim), at<double>(bc, c.key), nullptr,
                                      out_idx + (size_t)u0 * P, out_sim + (size_t)u0 * P, out_cnt + u0,
                                      at<int32_t>(bc, c.replay), replay_count, false)) ||
            (rc = launch_lshpc_collect(s, kept, n, u0, at<int32_t>(bc, c.replay), replay_count, handed_dev,
                                       handed_count)))
            return rc;
    }
    unsigned int nh = 0;
    const D2H rd{&nh, handed_count, sizeof(nh)};
    if ((rc = d2h_batch(ctx, &rd, 1))) return rc;
    handed.resize(nh);
    const D2H rl{handed.data(), handed_dev, 4 * (size_t)nh};
    if (nh && (rc = d2h_batch(ctx, &rl, 1))) return rc;
    std::sort(handed.begin(), handed.end());
    return 0;
}

static void every_user(int64_t nq, std::vector<int32_t>& handed) {
    handed.resize((size_t)nq);
    for (int64_t q = 0; q < nq; q++) handed[q] = (int32_t)q;
}

extern "C" int lshkm_lsh_p_closest(lshkm_lsh lsh, const double* X, const double* U, int64_t nq, int32_t excl_lo,
                                   int32_t excl_hi, int P, int32_t* out_idx, double* out_sim, int32_t* out_cnt,
                                   int64_t* ncand) {
    LSHKM_CHECK(lsh && lsh->built, LSHKM_ERR_STATE, "index not built (lshkm_lsh_build)");
    LSHKM_CHECK(nq >= 0 && nq < (1ll << 31) && P >= 1 && excl_lo <= excl_hi, LSHKM_ERR_ARG,
                "bad arguments (P >= 1, excl_lo <= excl_hi)");
    if (nq == 0) return 0;
    LSHKM_CHECK(U && out_idx && out_sim && out_cnt && (X || lsh->N == 0), LSHKM_ERR_ARG, "bad arguments");
    lshkm_ctx ctx = lsh->ctx;
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t N = lsh->N;
    const int d = lsh->proj.d, L = lsh->proj.L, k = lsh->proj.k;
    const bool small_cap = test_switch("LSHKM_LSHPC_CAP", "small");
    const int64_t cand_cap = small_cap ? (int64_t)1 << 16 : LSHPC_CAND_CAP;
    unsigned long long* stats = (unsigned long long*)ctx->stats.p;
    int rc = 0;
    const StreamSyncOnExit sync_guard{s, &rc};           // a failed call leaves nothing running

    std::vector<int32_t> handed;
    if (lshpc_route(lsh->metric == LSHKM_METRIC_COSINE, d, L, k, P,
                    N == 0 || test_switch("LSHKM_LSHPC_PATH", "lists")) == LshpcRoute::lists) {
        every_user(nq, handed);
    } else {
        const ScreenJob job{X, U, N, nq, d, L, k, P, lsh->bucket.as<int32_t>(), excl_lo, excl_hi, nullptr};
        const int32_t* ucode = nullptr;
        const auto user_codes = [&](int32_t* ubucket) {
            return hash_rows(ctx, HM_LSH_COSINE, U, nq, lsh->proj, lsh->nb, nullptr, nullptr, ubucket, nullptr);
        };
        if ((rc = lshpc_screen_all(ctx, job, user_codes, small_cap, out_idx, out_sim, out_cnt, ncand, handed, &ucode)))
            return rc;
    }
    if ((rc = launch_lshpc_stats(s, stats, nq - (int64_t)handed.size(), (int64_t)handed.size())) ||
        (rc = lshpc_lists(lsh, X, U, handed, excl_lo, excl_hi, P, cand_cap, out_idx, out_sim, out_cnt, ncand)))
        return rc;
    if (hipStreamSynchronize(s) != hipSuccess) {             // the workspace is reused by the next call
        set_error("lshkm_lsh_p_closest: hipStreamSynchronize failed");
        return LSHKM_ERR_HIP;
    }
    return 0;
}

// --------------------------------- hypercube recommender: P closest from the cube
// lshkm_cube_p_closest. The lists path: lshkm_cube_query's
// kernels -> get_P_closest (with its replay) on the users of `list` (ascending),
// gathered, their vertices (uvert: every user's, from the one vertex pass of
// the call) gathered too, so that no coin is drawn here. A user's neighbour
// count is the sum of its probed buckets' lengths: the chunks (at most cand_cap
// candidate rows and CUBEPC_SLOT_CAP (user, mask) slots) are cut from exact
// counts, no sizing query.
constexpr int64_t CUBEPC_SLOT_CAP = (int64_t)1 << 24;
static int cubepc_lists(lshkm_cube cube, const double* X, const double* U, const int32_t* uvert,
                        const std::vector<int32_t>& list, int probes, int P, int64_t cand_cap, int32_t* out_idx,
                        double* out_sim, int32_t* out_cnt, int64_t* ncand) {
    lshkm_ctx ctx = cube->ctx;
    hipStream_t s = ctx->stream;
    const int64_t m_all = (int64_t)list.size(), N = cube->N;
    const int d = cube->proj.d;
    if (m_all == 0) return 0;
    const std::vector<int32_t> masks = probe_masks(probes, cube->k);
    const int64_t S = (int64_t)masks.size();
    Buf &bw = ctx->ws_lshpc[4], &bq = ctx->ws_lshpc[5], &bm = ctx->ws_lshpc[6];
    int rc;
    // masks | list | vg (int32) | nc (int64)
    const size_t oma = 0, oli = oma + lshpc_round256(4 * (size_t)S), ovg = oli + lshpc_round256(4 * (size_t)m_all),
                 onc = ovg + lshpc_round256(4 * (size_t)m_all);
    if ((rc = bm.reserve(onc + lshpc_round256(8 * (size_t)m_all)))) return rc;
    const int32_t *dmasks = at<int32_t>(bm, oma), *dlist = at<int32_t>(bm, oli), *vg = at<int32_t>(bm, ovg);
    const H2D up[2] = {{at<int32_t>(bm, oma), masks.data(), 4 * (size_t)S},
                       {at<int32_t>(bm, oli), list.data(), 4 * (size_t)m_all}};
    std::vector<int64_t> nc((size_t)m_all);
    const D2H rd{nc.data(), at<int64_t>(bm, onc), 8 * (size_t)m_all};
    if ((rc = h2d_batch(ctx, up, 2)) ||
        (rc = launch_cubepc_handed(s, uvert, dlist, m_all, dmasks, (int)S, cube->row_ptr.as<int64_t>(),
                                   at<int32_t>(bm, ovg), at<int64_t>(bm, onc))) ||
        (rc = d2h_batch(ctx, &rd, 1)))
        return rc;
    for (int64_t i0 = 0; i0 < m_all;) {
        int64_t n = 0, total = 0;
        while (i0 + n < m_all && (n == 0 || (total + nc[i0 + n] <= cand_cap && (n + 1) * S <= CUBEPC_SLOT_CAP)))
            total += nc[i0 + n++];
        // Ug | qptr | sizes | slot_off | scan (int64) | gsim | gcnt | gidx
        const size_t slots = (size_t)(n * S);
        const size_t oUg = 0, oq = oUg + lshpc_round256(8 * (size_t)n * d), osz = oq + lshpc_round256(8 * (size_t)(n + 1)),
                     oso = osz + lshpc_round256(8 * slots), osc = oso + lshpc_round256(8 * (slots + 1)),
                     ogs = osc + lshpc_round256(scan_ws_bytes((int64_t)slots)), ogc = ogs + lshpc_round256(8 * (size_t)n * P),
                     ogi = ogc + lshpc_round256(4 * (size_t)n), bytes = ogi + lshpc_round256(4 * (size_t)n * P);
        if ((rc = bw.reserve(bytes)) || (rc = bq.reserve(4 * (size_t)std::max<int64_t>(total, 1)))) return rc;
        double* Ug = at<double>(bw, oUg);
        int64_t* qptr = at<int64_t>(bw, oq);
        if ((rc = launch_lshpc_gather(s, U, d, dlist + i0, n, Ug)) ||
            (rc = launch_cube_query(s, vg + i0, n, dmasks, (int)S, cube->row_ptr.as<int64_t>(), cube->idx.as<int32_t>(),
                                    at<int64_t>(bw, osz), at<int64_t>(bw, oso), qptr, bq.as<int32_t>(),
                                    at<int64_t>(bw, osc))) ||
            (rc = p_closest_launch(ctx, X, N, d, Ug, n, qptr, bq.as<int32_t>(), total, P, at<int32_t>(bw, ogi),
                                   at<double>(bw, ogs), at<int32_t>(bw, ogc))) ||
            (rc = launch_lshpc_scatter(s, dlist + i0, n, P, at<int32_t>(bw, ogi), at<double>(bw, ogs),
                                       at<int32_t>(bw, ogc), qptr, out_idx, out_sim, out_cnt, ncand)))
            return rc;
        i0 += n;
    }
    return 0;
}

extern "C" int lshkm_cube_p_closest(lshkm_cube cube, const double* X, const double* U, int64_t nq, int probes, int P,
                                    int32_t* out_idx, double* out_sim, int32_t* out_cnt, int64_t* ncand) {
    LSHKM_CHECK(cube && cube->built, LSHKM_ERR_STATE, "cube not built (lshkm_cube_build)");
    LSHKM_CHECK(nq >= 0 && nq < (1ll << 31) && P >= 1, LSHKM_ERR_ARG, "bad arguments (P >= 1)");
    if (nq == 0) return 0;
    LSHKM_CHECK(U && out_idx && out_sim && out_cnt && (X || cube->N == 0), LSHKM_ERR_ARG, "bad arguments");
    lshkm_ctx ctx = cube->ctx;
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t N = cube->N;
    const int d = cube->proj.d, k = cube->k;
    const bool small_cap = test_switch("LSHKM_LSHPC_CAP", "small");
    const int64_t cand_cap = small_cap ? (int64_t)1 << 16 : LSHPC_CAND_CAP;
    unsigned long long* stats = (unsigned long long*)ctx->stats.p;
    int rc = 0;
    const StreamSyncOnExit sync_guard{s, &rc};           // a failed call leaves nothing running

    // every user's vertex once, by the query's own routine: the euclidean
    // cube's unseen coins are drawn here, in (user, f) order, and nowhere else
    const auto user_codes = [&](int32_t* vertex) { return cube_vertices(cube, U, nq, vertex); };
    std::vector<int32_t> handed;
    const int32_t* uvert = nullptr;
    if (cubepc_route(d, k, P, N == 0 || test_switch("LSHKM_LSHPC_PATH", "lists")) == LshpcRoute::lists) {
        Buf& bu = ctx->ws_lshpc[1];
        if ((rc = bu.reserve(4 * (size_t)nq)) || (rc = user_codes(bu.as<int32_t>()))) return rc;
        uvert = bu.as<int32_t>();
        every_user(nq, handed);
    } else {
        const CubeProbe probe = cubepc_probe(probes, k);
        const ScreenJob job{X, U, N, nq, d, 1, k, P, cube->vertex.as<int32_t>(), 0, 0, &probe};
        if ((rc = lshpc_screen_all(ctx, job, user_codes, small_cap, out_idx, out_sim, out_cnt, ncand, handed, &uvert)))
            return rc;
    }
    if ((rc = launch_lshpc_stats(s, stats, nq - (int64_t)handed.size(), (int64_t)handed.size())) ||
        (rc = cubepc_lists(cube, X, U, uvert, handed, probes, P, cand_cap, out_idx, out_sim, out_cnt, ncand)))
        return rc;
    if (hipStreamSynchronize(s) != hipSuccess) {             // the workspace is reused by the next call
        set_error("lshkm_cube_p_closest: hipStreamSynchronize failed");
        return LSHKM_ERR_HIP;
    }
    return 0;
}

// ------------------------------------------------ clustering recommender
// get_top_N_recom(neighbors, user, N), crypto_rec.hpp:327-345, over whole
// clusters (main.cpp:260-269, :353-373): lshkm_cluster_top_n, and its sharded
// phases (_sims + _chain, _terms + _chain_terms). recom_layout.h states the
// form rule and every workspace.
//
// Host view of one call's CSRs, read and validated once: hu = the users'
// clusters, each in [0, K) (the reference indexes clusters[user.getCluster()],
// main.cpp:261, :366: an ID outside the clusters is a caller error, not an
// empty neighbourhood); soff = the prefix of each user's member count on this
// shard; hup = the unknown-index CSR offsets; toff = the prefix of each user's
// term count (members x unknown indexes).
struct RecomOffsets {
    std::vector<int32_t> hu;
    std::vector<int64_t> soff, hup, toff;
    int64_t max_members = 0;          // the largest cluster
};

static int check_unknowns(const RecomJob& j, const RecomOffsets& o) {
    bool ok = o.hup[0] == 0;
    for (int64_t q = 0; q < j.nq && ok; q++) ok = o.hup[q + 1] >= o.hup[q];
    LSHKM_CHECK(ok, LSHKM_ERR_ARG, "bad unknown-index lists (unk_ptr must start at 0 and not decrease)");
    LSHKM_CHECK(o.hup[j.nq] == 0 || j.unk_idx, LSHKM_ERR_ARG, "unk_idx is NULL");
    return 0;
}

static int check_clusters(const RecomJob& j, const RecomOffsets& o) {
    for (int64_t q = 0; q < j.nq; q++)
        LSHKM_CHECK(o.hu[q] >= 0 && o.hu[q] < j.K, LSHKM_ERR_ARG, "ucl holds a cluster ID outside [0, K)");
    return 0;
}

// From the cluster CSR and the users' clusters on the device: one batch of
// copies, one synchronisation. unknowns = false (lshkm_cluster_sims): the
// unknown-index lists are not read.
static int recom_offsets(lshkm_ctx ctx, const RecomJob& j, bool unknowns, RecomOffsets& o) {
    const int64_t nq = j.nq;
    std::vector<int64_t> hc((size_t)j.K + 1);
    o.hu.resize((size_t)nq);
    o.hup.assign((size_t)nq + 1, 0);
    const D2H rd[3] = {{hc.data(), j.crow, sizeof(int64_t) * (j.K + 1)},
                       {o.hu.data(), j.ucl, sizeof(int32_t) * nq},
                       {o.hup.data(), j.unk_ptr, unknowns ? sizeof(int64_t) * (nq + 1) : 0}};
    int rc;
    if ((rc = d2h_batch(ctx, rd, 3)) || (rc = check_clusters(j, o))) return rc;
    bool ok = hc[0] == 0;
    for (int c = 0; c < j.K && ok; c++) {
        ok = hc[c + 1] >= hc[c];
        o.max_members = std::max<int64_t>(o.max_members, hc[c + 1] - hc[c]);
    }
    LSHKM_CHECK(ok && hc[j.K] <= j.N, LSHKM_ERR_ARG,
                "bad cluster CSR (crow must start at 0, not decrease, and hold at most N members)");
    LSHKM_CHECK(hc[j.K] == 0 || j.crows, LSHKM_ERR_ARG, "crows is NULL");
    LSHKM_CHECK(o.max_members < (1ll << 31), LSHKM_ERR_ARG, "a cluster of 2^31 members or more");
    if ((rc = check_unknowns(j, o))) return rc;
    o.soff.assign((size_t)nq + 1, 0);
    o.toff.assign((size_t)nq + 1, 0);
    for (int64_t q = 0; q < nq; q++) {
        const int64_t n = hc[o.hu[q] + 1] - hc[o.hu[q]];
        o.soff[q + 1] = o.soff[q] + n;
        o.toff[q + 1] = o.toff[q] + n * (o.hup[q + 1] - o.hup[q]);
    }
    return 0;
}

// Read back from the device, for the public chain phases (their callers hold
// only device arrays): ucl where the job has one, soff / toff where given.
static int recom_offsets_device(lshkm_ctx ctx, const RecomJob& j, const int64_t* soff, const int64_t* toff,
                                RecomOffsets& o) {
    const size_t n1 = (size_t)j.nq + 1;
    o.hu.resize(j.ucl ? (size_t)j.nq : 0);
    o.hup.resize(n1);
    o.soff.resize(toff ? n1 : 0);
    o.toff.resize(toff ? n1 : 0);
    const D2H rd[4] = {{o.hu.data(), j.ucl, sizeof(int32_t) * o.hu.size()},
                       {o.soff.data(), soff, sizeof(int64_t) * o.soff.size()},
                       {o.toff.data(), toff, sizeof(int64_t) * o.toff.size()},
                       {o.hup.data(), j.unk_ptr, sizeof(int64_t) * n1}};
    int rc;
    if ((rc = d2h_batch(ctx, rd, 4)) || (j.ucl && (rc = check_clusters(j, o)))) return rc;
    return check_unknowns(j, o);
}

// What one entry point asks of recom_cluster. soff / toff / sims / terms: the
// caller's device arrays, written by SIMS / TERMS (when the totals fit cap /
// tcap; the totals go to *total / *tterms either way) and only read by CHAIN /
// CHAIN_TERMS, as carry_in is. out != NULL: the final step; else the running
// sums go to carry_out.
struct RecomRequest {
    enum Op { TOP_N, SIMS, TERMS, CHAIN, CHAIN_TERMS } op;
    int64_t *soff, *toff;
    double *sims, *terms;
    int64_t cap, tcap;
    int64_t *total, *tterms;
    RecomCarry carry_in, carry_out;
    int n_top;
    int32_t* out;
};
template <typename T> static T* read_only(const T* p) { return const_cast<T*>(p); }

// Phase 1 of the terms form: the offsets up, then, when the caller's arrays
// hold them, every similarity and term of this shard.
static int recom_terms(lshkm_ctx ctx, const RecomJob& j, const RecomOffsets& o, const RecomRequest& r,
                       unsigned long long* soft) {
    const int64_t nq = j.nq, S = o.soff[nq];
    const H2D offs[2] = {{r.soff, o.soff.data(), sizeof(int64_t) * (nq + 1)},
                         {r.toff, o.toff.data(), sizeof(int64_t) * (nq + 1)}};
    if (!(r.sims && r.terms && S <= r.cap && o.toff[nq] <= r.tcap && S > 0)) return h2d_batch(ctx, offs, 2);
    Buf &map = ctx->ws_call[8], &gb = ctx->ws_call[9];
    const RcWorkList w = rc_work_list(o.hu, o.soff);         // staged by h2d_batch
    const RcPackLayout pl = rc_pack_layout(w.pack.size(), w.nitems, w.nusers);
    int rc;
    if ((rc = map.reserve(rc_map_layout(S, nq).bytes)) || (rc = gb.reserve(pl.bytes))) return rc;
    int32_t* dp = at<int32_t>(gb, pl.pack);
    const H2D up[3] = {offs[0], offs[1], {dp, w.pack.data(), 4 * w.pack.size()}};
    if ((rc = h2d_batch(ctx, up, 3))) return rc;
    const RcGroups groups{dp, w.ngroups, w.nitems, dp + w.gcl(), dp + w.gptr(), dp + w.gusr(),
                          at<char>(gb, pl.items), w.nusers, at<char>(gb, pl.users)};
    // no host synchronisation: the uploads are staged (h2d_batch), the outputs
    // and the workspaces are ordered on the stream
    return launch_rc_terms(ctx->stream, j, RcTermsOut{r.soff, r.toff, S, r.sims, r.terms}, map.as<char>(), groups, soft);
}

// Phase 2 of the terms form: the chains from the stored terms, continued from
// `in`, into `carry_to` or (the final step) `out`.
static int recom_chain_terms(lshkm_ctx ctx, const RecomJob& j, const RecomOffsets& o, const RcTermsOut& t,
                             const RecomCarry& in, const RecomCarry& carry_to, const RecomOut& out) {
    // users whose cluster holds >= RC_LONG_MIN members here: their chains by
    // binade segments, in batches (rc_long_batches)
    std::vector<RcLongUser> lus;
    for (int64_t q = 0; q < j.nq; q++) {
        const int64_t n = o.soff[q + 1] - o.soff[q];
        if (n >= RC_LONG_MIN)
            lus.push_back(RcLongUser{q, n, o.soff[q], o.toff[q], o.hup[q], o.hup[q + 1] - o.hup[q], 0, 0});
    }
    std::vector<int64_t> hcrow;                         // staged by h2d_batch with the user table
    const std::vector<RcLongBatch> batches = rc_long_batches(lus);
    int rc;
    for (const RcLongBatch& b : batches) {
        const int64_t nl = (int64_t)(b.k1 - b.k0);
        hcrow.assign(1, 0);
        for (size_t k = b.k0; k < b.k1; k++) {
            lus[k].off = hcrow.back();
            hcrow.push_back(hcrow.back() + lus[k].n);
        }
        const RcLongLayout ll = rc_long_layout(b.rows, nl, b.D, seg_columns_ws_bytes(b.rows, (int)nl, (int)b.D));
        Buf& wl = ctx->ws_long;
        if ((rc = wl.reserve(ll.bytes))) return rc;
        RcLongUser* tab = at<RcLongUser>(wl, ll.tab);
        int64_t* crow = at<int64_t>(wl, ll.crow);
        const H2D up[2] = {{tab, lus.data() + b.k0, (size_t)nl * sizeof(RcLongUser)},
                           {crow, hcrow.data(), (size_t)(nl + 1) * 8}};
        if ((rc = h2d_batch(ctx, up, 2))) return rc;
        const RcLong L{tab, nl, b.rows, (int)b.D, crow, at<double>(wl, ll.V), at<double>(wl, ll.carry),
                       at<double>(wl, ll.sums), at<int32_t>(wl, ll.iota), at<char>(wl, ll.ws)};
        if ((rc = launch_rc_long(ctx->stream, t, in, j.u_mean, carry_to, out.pred, L))) return rc;
        // a further batch may grow ws_long: not while this one's kernels run
        if (&b != &batches.back()) LSHKM_HIP(hipStreamSynchronize(ctx->stream));
    }
    if ((rc = launch_rc_chain_terms(ctx->stream, j, t, in, carry_to, out.pred, lus.empty() ? INT64_MAX : RC_LONG_MIN)))
        return rc;
    // no host synchronisation: the pred / pidx workspace's next user is ordered
    // on the same stream (a reserve that grows it frees through hipFree)
    return out.out ? launch_rc_top(ctx->stream, j, t.soff, in.cnt, out) : 0;
}

// The one owner of a clustering-recommender call: the route (recom_route), the
// reservations of ws_call[0, 1, 2, 5 .. 9] and ws_long, the uploads, the
// launches and the end-of-call ordering.
static int recom_cluster(lshkm_ctx ctx, const RecomJob& j, const RecomRequest& r) {
    using R = RecomRequest;
    const bool chain = r.op == R::CHAIN || r.op == R::CHAIN_TERMS;
    const bool rows_ok = j.X.p && j.crow && j.ucl && j.N >= 1 && j.d >= 1 && j.K >= 1;
    bool ok = ctx && j.unk_ptr && j.nq >= 0 && r.n_top >= 0 && (r.op == R::CHAIN_TERMS || rows_ok);
    switch (r.op) {
        case R::TOP_N: ok = ok && j.x_mean && j.U.p && j.u_mean && r.out; break;
        case R::SIMS: ok = ok && j.U.p && r.soff && r.total && r.cap >= 0; break;
        case R::TERMS:
            ok = ok && j.x_mean && j.U.p && r.soff && r.toff && r.total && r.tterms && r.cap >= 0 && r.tcap >= 0;
            break;
        case R::CHAIN: ok = ok && j.x_mean && j.u_mean && r.soff; break;
        case R::CHAIN_TERMS: ok = ok && j.u_mean && r.soff && r.toff; break;
    }
    LSHKM_CHECK(ok, LSHKM_ERR_ARG, "bad arguments");
    if (chain) {
        const RecomCarry &ci = r.carry_in, &co = r.carry_out;
        LSHKM_CHECK((ci.main == nullptr) == (ci.abs == nullptr) && (ci.abs == nullptr) == (ci.cnt == nullptr),
                    LSHKM_ERR_ARG, "carry_main / carry_abs / carry_cnt: all or none");
        LSHKM_CHECK(r.out || (co.main && co.abs && co.cnt), LSHKM_ERR_ARG, "either the carry outputs or out");
    }
    LSHKM_CHECK(r.op != R::TERMS || recom_route(j.d, j.X.f64, 0) == RecomRoute::terms, LSHKM_ERR_ARG,
                "the terms form stages rows of a multiple of 8 B up to " + std::to_string(RC_ROW_MAX) +
                    " B (use lshkm_cluster_sims)");
    if ((r.op == R::TOP_N && (j.nq == 0 || r.n_top == 0)) || (chain && j.nq == 0)) return 0;
    LSHKM_HIP(hipSetDevice(ctx->device));

    int rc = 0;
    const StreamSyncOnExit sync_guard{ctx->stream, &rc};     // a failed call leaves nothing running
    RecomOffsets o;
    if ((rc = chain ? recom_offsets_device(ctx, j, r.op == R::CHAIN_TERMS ? r.soff : nullptr,
                                           r.op == R::CHAIN_TERMS ? r.toff : nullptr, o)
                    : recom_offsets(ctx, j, r.op != R::SIMS, o)))
        return rc;
    const int64_t nq = j.nq, S = chain ? 0 : o.soff[nq], T = chain ? 0 : o.toff[nq];
    // the final step's predictions, or the running sums carried on: one or the other
    const bool final_step = r.out != nullptr;
    const RecomCarry carry_to = final_step ? RecomCarry{} : r.carry_out;
    RecomOut out{};
    if (final_step) {
        Buf &pred = ctx->ws_call[1], &pidx = ctx->ws_call[2];
        const size_t M = (size_t)std::max<int64_t>(o.hup[nq], 1);
        if ((rc = pred.reserve(sizeof(double) * M)) || (rc = pidx.reserve(sizeof(int32_t) * M))) return rc;
        out = RecomOut{pred.as<double>(), pidx.as<int32_t>(), r.n_top, r.out};
    }
    unsigned long long* soft = (unsigned long long*)ctx->stats.p + STAT_REC_SOFT;
    switch (r.op) {
        case R::TOP_N: {
            if (recom_route(j.d, j.X.f64, T) == RecomRoute::terms) {
                Buf &bs = ctx->ws_call[0], &bt = ctx->ws_call[5], &bso = ctx->ws_call[6], &bto = ctx->ws_call[7];
                if ((rc = bs.reserve(8 * (size_t)std::max<int64_t>(S, 1))) ||
                    (rc = bt.reserve(8 * (size_t)std::max<int64_t>(T, 1))) ||
                    (rc = bso.reserve(8 * (size_t)(nq + 1))) || (rc = bto.reserve(8 * (size_t)(nq + 1))))
                    return rc;
                R t = r;
                t.soff = bso.as<int64_t>(), t.toff = bto.as<int64_t>();
                t.sims = bs.as<double>(), t.terms = bt.as<double>();
                t.cap = S, t.tcap = T;
                if ((rc = recom_terms(ctx, j, o, t, soft))) return rc;
                return rc = recom_chain_terms(ctx, j, o, RcTermsOut{t.soff, t.toff, S, t.sims, t.terms}, RecomCarry{},
                                              carry_to, out);
            }
            // one wave per user; ws_call[0] is the terms form's similarities otherwise
            const RcWaveScratch ws = rc_wave_scratch(nq, o.max_members);
            Buf& scratch = ctx->ws_call[0];
            if ((rc = scratch.reserve(ws.bytes)) ||
                (rc = launch_rc_cluster_top_n(ctx->stream, j, scratch.as<double>(), ws, out, soft)))
                return rc;
            break;
        }
        case R::SIMS: {
            *r.total = S;
            const H2D up{r.soff, o.soff.data(), sizeof(int64_t) * (nq + 1)};
            if ((rc = h2d_batch(ctx, &up, 1))) return rc;
            if (r.sims && S <= r.cap && S > 0 && (rc = launch_rc_shard_sims(ctx->stream, j, r.soff, r.sims, soft)))
                return rc;
            break;
        }
        case R::TERMS:
            *r.total = S;
            *r.tterms = T;
            return rc = recom_terms(ctx, j, o, r, soft);
        case R::CHAIN:
            if ((rc = launch_rc_shard_chain(ctx->stream, j, r.soff, r.sims, r.carry_in, carry_to, out))) return rc;
            if (!final_step) return 0;
            break;
        case R::CHAIN_TERMS:
            return rc = recom_chain_terms(ctx, j, o, RcTermsOut{r.soff, r.toff, o.soff[nq], r.sims, r.terms},
                                          r.carry_in, carry_to, out);
    }
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is reused by the next call
    return 0;
}

// The request of an entry point that ends in (or is) a chain phase: the arrays
// it only reads, the carry in and out, the final step's n_top / out.
static RecomRequest chain_request(RecomRequest::Op op, const int64_t* soff, const int64_t* toff, const double* sims,
                                  const double* terms, const double* cm, const double* ca, const int64_t* cc,
                                  double* mo, double* ao, int64_t* co, int n_top, int32_t* out) {
    return {op, read_only(soff), read_only(toff), read_only(sims), read_only(terms), 0, 0, nullptr, nullptr,
            {read_only(cm), read_only(ca), read_only(cc)}, {mo, ao, co}, n_top, out};
}

extern "C" {

int lshkm_cluster_terms_supported(int d, int f64) { return recom_route(d, f64 != 0, 0) == RecomRoute::terms; }

int lshkm_cluster_sims(lshkm_ctx ctx, const float* X, int64_t N, int d, const int64_t* crow, const int32_t* crows,
                       int K, const float* U, int64_t nq, const int32_t* ucl, const int64_t* unk_ptr,
                       int64_t* soff, double* sims, int64_t cap, int64_t* total) {
    return recom_cluster(ctx, {X, nullptr, N, d, crow, crows, K, U, nullptr, nq, ucl, unk_ptr, nullptr},
                         {RecomRequest::SIMS, soff, nullptr, sims, nullptr, cap, 0, total});
}

int lshkm_cluster_sims_f64(lshkm_ctx ctx, const double* X, int64_t N, int d, const int64_t* crow,
                           const int32_t* crows, int K, const double* U, int64_t nq, const int32_t* ucl,
                           const int64_t* unk_ptr, int64_t* soff, double* sims, int64_t cap, int64_t* total) {
    return recom_cluster(ctx, {X, nullptr, N, d, crow, crows, K, U, nullptr, nq, ucl, unk_ptr, nullptr},
                         {RecomRequest::SIMS, soff, nullptr, sims, nullptr, cap, 0, total});
}

int lshkm_cluster_chain(lshkm_ctx ctx, const float* X, const double* x_mean, int64_t N, int d, const int64_t* crow,
                        const int32_t* crows, int K, int64_t nq, const int32_t* ucl, const double* u_mean,
                        const int64_t* unk_ptr, const int32_t* unk_idx, const int64_t* soff, const double* sims,
                        const double* carry_main, const double* carry_abs, const int64_t* carry_cnt,
                        double* main_out, double* abs_out, int64_t* cnt_out, int n_top, int32_t* out) {
    return recom_cluster(ctx, {X, x_mean, N, d, crow, crows, K, Pts(), u_mean, nq, ucl, unk_ptr, unk_idx},
                         chain_request(RecomRequest::CHAIN, soff, nullptr, sims, nullptr, carry_main, carry_abs, carry_cnt,
                                       main_out, abs_out, cnt_out, n_top, out));
}

int lshkm_cluster_chain_f64(lshkm_ctx ctx, const double* X, const double* x_mean, int64_t N, int d,
                            const int64_t* crow, const int32_t* crows, int K, int64_t nq, const int32_t* ucl,
                            const double* u_mean, const int64_t* unk_ptr, const int32_t* unk_idx, const int64_t* soff,
                            const double* sims, const double* carry_main, const double* carry_abs,
                            const int64_t* carry_cnt, double* main_out, double* abs_out, int64_t* cnt_out, int n_top,
                            int32_t* out) {
    return recom_cluster(ctx, {X, x_mean, N, d, crow, crows, K, Pts(), u_mean, nq, ucl, unk_ptr, unk_idx},
                         chain_request(RecomRequest::CHAIN, soff, nullptr, sims, nullptr, carry_main, carry_abs, carry_cnt,
                                       main_out, abs_out, cnt_out, n_top, out));
}

int lshkm_cluster_terms(lshkm_ctx ctx, const float* X, const double* x_mean, int64_t N, int d, const int64_t* crow,
                        const int32_t* crows, int K, const float* U, int64_t nq, const int32_t* ucl,
                        const int64_t* unk_ptr, const int32_t* unk_idx, int64_t* soff, int64_t* toff, double* sims,
                        double* terms, int64_t cap, int64_t tcap, int64_t* total, int64_t* tterms) {
    return recom_cluster(ctx, {X, x_mean, N, d, crow, crows, K, U, nullptr, nq, ucl, unk_ptr, unk_idx},
                         {RecomRequest::TERMS, soff, toff, sims, terms, cap, tcap, total, tterms});
}

int lshkm_cluster_terms_f64(lshkm_ctx ctx, const double* X, const double* x_mean, int64_t N, int d,
                            const int64_t* crow, const int32_t* crows, int K, const double* U, int64_t nq,
                            const int32_t* ucl, const int64_t* unk_ptr, const int32_t* unk_idx, int64_t* soff,
                            int64_t* toff, double* sims, double* terms, int64_t cap, int64_t tcap, int64_t* total,
                            int64_t* tterms) {
    return recom_cluster(ctx, {X, x_mean, N, d, crow, crows, K, U, nullptr, nq, ucl, unk_ptr, unk_idx},
                         {RecomRequest::TERMS, soff, toff, sims, terms, cap, tcap, total, tterms});
}

int lshkm_cluster_chain_terms(lshkm_ctx ctx, int64_t nq, const double* u_mean, const int64_t* unk_ptr,
                              const int32_t* unk_idx, const int64_t* soff, const int64_t* toff, const double* sims,
                              const double* terms, const double* carry_main, const double* carry_abs,
                              const int64_t* carry_cnt, double* main_out, double* abs_out, int64_t* cnt_out,
                              int n_top, int32_t* out) {
    return recom_cluster(ctx, {Pts(), nullptr, 0, 0, nullptr, nullptr, 0, Pts(), u_mean, nq, nullptr, unk_ptr, unk_idx},
                         chain_request(RecomRequest::CHAIN_TERMS, soff, toff, sims, terms, carry_main, carry_abs, carry_cnt,
                                       main_out, abs_out, cnt_out, n_top, out));
}

int lshkm_cluster_top_n(lshkm_ctx ctx, const float* X, const double* x_mean, int64_t N, int d, const int64_t* crow,
                        const int32_t* crows, int K, const float* U, const double* u_mean, int64_t nq,
                        const int32_t* ucl, const int64_t* unk_ptr, const int32_t* unk_idx, int n_top, int32_t* out) {
    return recom_cluster(ctx, {X, x_mean, N, d, crow, crows, K, U, u_mean, nq, ucl, unk_ptr, unk_idx},
                         chain_request(RecomRequest::TOP_N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, nullptr, n_top, out));
}

int lshkm_cluster_top_n_f64(lshkm_ctx ctx, const double* X, const double* x_mean, int64_t N, int d,
                            const int64_t* crow, const int32_t* crows, int K, const double* U, const double* u_mean,
                            int64_t nq, const int32_t* ucl, const int64_t* unk_ptr, const int32_t* unk_idx, int n_top,
                            int32_t* out) {
    return recom_cluster(ctx, {X, x_mean, N, d, crow, crows, K, U, u_mean, nq, ucl, unk_ptr, unk_idx},
                         chain_request(RecomRequest::TOP_N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, nullptr, n_top, out));
}

}  // extern "C"

// ------------------------------------------------- recommender validation
// glibc's rand() after srand(seed) (random_r.c, TYPE_3: the additive feedback
// generator x^31 + x^3 + 1), restated: r[0] = seed (0 -> 1), r[i] =
// 16807 * r[i-1] mod 2147483647 for i < 31 (Schrage's form on int32),
// r[i] = r[i-31] + r[i-3] afterwards (r[31..33] = r[0..2]), the first 310
// outputs discarded: draw n is r[344 + n] >> 1. Slot i % 31 holds r[i].
namespace {
struct GlibcRand {
    uint32_t buf[31];
    int64_t i;
    explicit GlibcRand(uint64_t seed64) {
        uint32_t seed = (uint32_t)seed64;
        if (seed == 0) seed = 1;
        int32_t word = (int32_t)seed;
        buf[0] = (uint32_t)word;
        for (int j = 1; j < 31; j++) {
            const long hi = word / 127773, lo = word % 127773;
            long w = 16807 * lo - 2836 * hi;
            if (w < 0) w += 2147483647;
            word = (int32_t)w;
            buf[j] = (uint32_t)word;
        }
        for (i = 34; i < 344; i++) buf[i % 31] += buf[(i - 3) % 31];
    }
    int32_t next() {
        const uint32_t v = (buf[i % 31] += buf[(i - 3) % 31]);
        i++;
        return (int32_t)(v >> 1);
    }
};

// split_to_10 (crypto_rec.hpp:348-367): rows [10][N / 10]. A Fenwick tree of
// the remaining positions finds the rand_i-th remaining user (what
// input_vectors[rand_i] is after the erases before it).
void split10(uint64_t seed, int64_t N, int32_t* rows) {
    const int64_t F = N / 10;
    if (F == 0) return;
    GlibcRand g(seed);
    std::vector<int32_t> tree((size_t)N + 1, 0);
    for (int64_t p = 1; p <= N; p++) {
        tree[p] += 1;
        const int64_t up = p + (p & -p);
        if (up <= N) tree[up] += tree[p];
    }
    int64_t top = 1;
    while (top * 2 <= N) top *= 2;
    int64_t remaining = N;
    for (int64_t m = 0; m < 10 * F; m++) {
        int64_t want = (int64_t)((uint64_t)g.next() % (uint64_t)remaining);   // 0-based rank among the remaining
        int64_t pos = 0;
        for (int64_t step = top; step > 0; step >>= 1)
            if (pos + step <= N && tree[pos + step] <= want) {
                pos += step;
                want -= tree[pos];
            }
        rows[m] = (int32_t)pos;                                                // 0-based user (tree position pos + 1)
        for (int64_t p = pos + 1; p <= N; p += p & -p) tree[p] -= 1;
        remaining--;
    }
}

struct LshHandles {
    std::vector<lshkm_lsh> h;
    ~LshHandles() {
        for (lshkm_lsh x : h) (void)lshkm_lsh_destroy(x);
    }
};
}  // namespace

extern "C" {

int lshkm_cv_split10(uint64_t seed, int64_t N, int32_t* rows) {
    LSHKM_CHECK(N >= 0 && N < (1ll << 31) && (rows || N < 10), LSHKM_ERR_ARG, "bad arguments");
    split10(seed, N, rows);
    return 0;
}

int lshkm_cv_draws(const uint64_t* seed, int64_t n, int64_t per, int32_t* draw) {
    LSHKM_CHECK(n >= 0 && per >= 0 && (n * per == 0 || (seed && draw)), LSHKM_ERR_ARG, "bad arguments");
    for (int64_t i = 0; i < n; i++) {
        GlibcRand g(seed[i]);
        for (int64_t j = 0; j < per; j++) draw[i * per + j] = g.next();
    }
    return 0;
}

int lshkm_cv_hide(lshkm_ctx ctx, const double* X, const double* x_mean, int64_t N, int d, const int64_t* unk_ptr,
                  const int32_t* unk_idx, const int32_t* draw, double* H, double* h_mean, int32_t* hide_idx,
                  double* old) {
    LSHKM_CHECK(ctx && N >= 0 && d >= 1 && (N == 0 || (X && x_mean && unk_ptr && draw && H && h_mean && hide_idx && old)),
                LSHKM_ERR_ARG, "bad arguments");
    LSHKM_HIP(hipSetDevice(ctx->device));
    return launch_cv_hide(ctx->stream, X, x_mean, nullptr, N, d, unk_ptr, unk_idx, draw, H, h_mean, hide_idx, old);
}

int lshkm_cv_exclude(lshkm_ctx ctx, const int64_t* in_ptr, const int32_t* in_idx, int64_t nq, int32_t lo, int32_t hi,
                     int64_t* out_ptr, int32_t* out_idx) {
    LSHKM_CHECK(ctx && in_ptr && out_ptr && nq >= 0 && lo <= hi && (out_idx == nullptr || out_idx != in_idx),
                LSHKM_ERR_ARG, "bad arguments");
    LSHKM_HIP(hipSetDevice(ctx->device));
    Buf &cnt = ctx->ws_call[6], &ra = ctx->ws_call[7], &rb = ctx->ws_call[8];
    const size_t n = (size_t)std::max<int64_t>(nq, 1);
    int rc;
    if ((rc = cnt.reserve(8 * n)) || (rc = ra.reserve(4 * n)) || (rc = rb.reserve(4 * n))) return rc;
    return launch_cv_exclude(ctx->stream, in_ptr, in_idx, nq, lo, hi, cnt.as<int64_t>(), ra.as<int32_t>(),
                             rb.as<int32_t>(), out_ptr, out_idx);
}

int lshkm_predicted_scores(lshkm_ctx ctx, const double* X, const double* x_mean, int64_t N, int d, const double* u_mean,
                           int64_t nq, const int64_t* unk_ptr, const int32_t* unk_idx, const int32_t* nb_idx,
                           const double* nb_sim, const int32_t* nb_cnt, int P, double* pred) {
    LSHKM_CHECK(ctx && X && x_mean && u_mean && unk_ptr && nb_idx && nb_sim && nb_cnt && N >= 1 && d >= 1 && nq >= 0 &&
                    P >= 1,
                LSHKM_ERR_ARG, "bad arguments");
    if (nq == 0) return 0;
    LSHKM_HIP(hipSetDevice(ctx->device));
    int64_t total = 0;
    int rc;
    if ((rc = read_i64(ctx, unk_ptr + nq, &total))) return rc;
    LSHKM_CHECK(total >= 0 && (total == 0 || (unk_idx && pred)), LSHKM_ERR_ARG, "bad unknown-index lists");
    return launch_cv_predict(ctx->stream, X, x_mean, d, u_mean, nq, total, unk_ptr, unk_idx, nb_idx, nb_sim, nb_cnt, P,
                             pred);
}

int lshkm_cv_fold_sum(lshkm_ctx ctx, int64_t nq, const int32_t* hide_idx, const double* old, const double* pred,
                      const int64_t* nb_ptr, double* err, double* k_sum, int64_t* count) {
    LSHKM_CHECK(ctx && nq >= 0 && k_sum && count && (nq == 0 || (hide_idx && old && pred && nb_ptr)), LSHKM_ERR_ARG,
                "bad arguments");
    LSHKM_HIP(hipSetDevice(ctx->device));
    return launch_cv_fold_sum(ctx->stream, nq, hide_idx, old, pred, nb_ptr, err, k_sum, count, false);
}

int lshkm_lsh_validate10(lshkm_ctx ctx, const double* X, const double* x_mean, int64_t N, int d, const int64_t* unk_ptr,
                         const int32_t* unk_idx, int metric, int k, int L, int lsh_bucket_div, float w, int P,
                         uint64_t split_seed, uint64_t hide_seed, const uint64_t* hide_seeds, const uint64_t* lsh_seeds,
                         double* mae_host, double* fold_sum_host, int64_t* fold_cnt_host, double* err_dev) {
    LSHKM_CHECK(ctx && mae_host && N >= 0 && N < (1ll << 31), LSHKM_ERR_ARG, "bad arguments");
    LSHKM_CHECK(P >= 1 && d >= 1, LSHKM_ERR_ARG, "P and d must be >= 1");
    LSHKM_CHECK(metric == LSHKM_METRIC_EUCLIDEAN || metric == LSHKM_METRIC_COSINE, LSHKM_ERR_ARG, "unknown metric");
    const int64_t F = N / 10, M = 10 * F;
    int64_t nb = 0;
    if (metric == LSHKM_METRIC_EUCLIDEAN) {
        LSHKM_CHECK(lsh_bucket_div >= 1, LSHKM_ERR_ARG, "lsh_bucket_div must be >= 1");
        nb = (M - F) / lsh_bucket_div;                   // pool.size() / lsh_bucket_div (lsh_cube.hpp:52)
        LSHKM_CHECK(nb >= 1, LSHKM_ERR_ARG, "pool size / lsh_bucket_div is 0 buckets (the reference divides by zero)");
    }
    if (F == 0) {                                        // every fold is empty: calc_user_num stays 0
        *mae_host = 0.0;
        for (int i = 0; i < 10; i++) {
            if (fold_sum_host) fold_sum_host[i] = 0.0;
            if (fold_cnt_host) fold_cnt_host[i] = 0;
        }
        return 0;
    }
    LSHKM_CHECK(X && x_mean && unk_ptr && lsh_seeds, LSHKM_ERR_ARG, "bad arguments");
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;

    // host: the split and every user's hide draw, in split order
    std::vector<int32_t> rows((size_t)M), draw((size_t)M);
    split10(split_seed, N, rows.data());
    const int32_t draw_all = GlibcRand(hide_seed).next();
    for (int64_t m = 0; m < M; m++) draw[m] = hide_seeds ? GlibcRand(hide_seeds[rows[m]]).next() : draw_all;

    // ten index handles up front (their parameter uploads wait for the stream)
    LshHandles tabs;
    {
        std::vector<float> V, t;
        std::vector<int32_t> r;
        std::vector<double> R;
        const size_t lk = (size_t)L * k;
        LSHKM_CHECK(k >= 1 && L >= 1, LSHKM_ERR_ARG, "k and L must be >= 1");
        if (metric == LSHKM_METRIC_EUCLIDEAN) { V.resize(lk * d); t.resize(lk); r.resize(lk); }
        else R.resize(lk * d);
        for (int i = 0; i < 10; i++) {
            uint32_t st = 0;
            if (metric == LSHKM_METRIC_EUCLIDEAN)
                rc = lshkm_params_lsh_euclidean(lsh_seeds[i], L, k, d, w, V.data(), t.data(), r.data(), &st);
            else
                rc = lshkm_params_lsh_cosine(lsh_seeds[i], L, k, d, R.data(), &st);
            if (rc) return rc;
            lshkm_lsh h = nullptr;
            if ((rc = lshkm_lsh_create(ctx, metric, d, k, L, nb, w, V.data(), t.data(), r.data(), R.data(), &h)))
                return rc;
            tabs.h.push_back(h);
        }
    }

    // device state: W (the working matrix, split order) and the hidden forms
    Buf bW, bWm, bH, bHm, bhide, bold, brows, bdraw, bpred, bhptr, bsum, bcnt, bqptr, bqidx, beptr, beidx, bscr, bra, brb,
        bnidx, bnsim, bncnt;
    const StreamSyncOnExit sync_guard{s};            // the buffers above are freed after the stream drained
    const size_t Md = (size_t)M * d;
    if ((rc = bW.reserve(8 * Md)) || (rc = bWm.reserve(8 * M)) || (rc = bH.reserve(8 * Md)) ||
        (rc = bHm.reserve(8 * M)) || (rc = bhide.reserve(4 * M)) || (rc = bold.reserve(8 * M)) ||
        (rc = brows.reserve(4 * M)) || (rc = bdraw.reserve(4 * M)) || (rc = bpred.reserve(8 * M)) ||
        (rc = bhptr.reserve(8 * (M + 1))) || (rc = bsum.reserve(8 * 10)) || (rc = bcnt.reserve(8 * 10)) ||
        (rc = bqptr.reserve(8 * (F + 1))) || (rc = beptr.reserve(8 * (F + 1))) || (rc = bscr.reserve(8 * F)) ||
        (rc = bra.reserve(4 * F)) || (rc = brb.reserve(4 * F)) || (rc = bnidx.reserve(4 * (size_t)F * P)) ||
        (rc = bnsim.reserve(8 * (size_t)F * P)) || (rc = bncnt.reserve(4 * F)))
        return rc;
    std::vector<int64_t> hptr((size_t)M + 1);        // every user's one-element unknown list {hide_idx}
    for (int64_t m = 0; m <= M; m++) hptr[m] = m;
    const H2D up[3] = {{brows.p, rows.data(), 4 * (size_t)M},
                       {bdraw.p, draw.data(), 4 * (size_t)M},
                       {bhptr.p, hptr.data(), 8 * (size_t)(M + 1)}};
    if ((rc = h2d_batch(ctx, up, 3))) return rc;
    double *W = bW.as<double>(), *Wm = bWm.as<double>(), *H = bH.as<double>(), *Hm = bHm.as<double>();
    int32_t* hide = bhide.as<int32_t>();
    if ((rc = launch_cv_gather(s, X, x_mean, brows.as<int32_t>(), M, d, W, Wm)) ||
        (rc = launch_cv_hide(s, X, x_mean, brows.as<int32_t>(), M, d, unk_ptr, unk_idx, bdraw.as<int32_t>(), H, Hm, hide,
                             bold.as<double>())))
        return rc;

    // candidate rows per chunk of queries: ~28 B of lists and workspace each
    const int64_t cand_cap = test_switch("LSHKM_CV_CHUNK", "small") ? 64 : (int64_t)1 << 28;
    // first guess from the mean bucket load (L tables of M / buckets rows each);
    // a chunk whose lists come out larger is cut down below
    const int64_t buckets = metric == LSHKM_METRIC_EUCLIDEAN ? nb : (int64_t)1 << std::min(k, 40);
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(F, cand_cap / std::max<int64_t>(1, (int64_t)L * (M / buckets + 1))));
    for (int i = 0; i < 10; i++) {
        const int64_t q0 = (int64_t)i * F;
        // fold i's users take their hidden form (main.cpp:407-410) for good:
        // they are the queries now and pool rows of the later folds
        LSHKM_HIP(hipMemcpyAsync(W + q0 * d, H + q0 * d, 8 * (size_t)F * d, hipMemcpyDeviceToDevice, s));
        LSHKM_HIP(hipMemcpyAsync(Wm + q0, Hm + q0, 8 * (size_t)F, hipMemcpyDeviceToDevice, s));
        // hashing is per row: one build over all M rows under fold i's
        // parameters serves the pool (slice i dropped from the results below)
        lshkm_lsh h = tabs.h[i];
        if ((rc = lshkm_lsh_build_f64(h, W, M))) return rc;
        // the held-out users in chunks whose candidate lists fit cand_cap rows
        // (the lists grow with N: a cosine bucket holds N / 2^k users per table)
        for (int64_t qb = 0; qb < F;) {
            const int64_t n = std::min(F - qb, chunk), u0 = q0 + qb;
            int64_t total = 0;
            if ((rc = lshkm_lsh_query_f64(h, W + u0 * d, n, nullptr, 1, bqptr.as<int64_t>(), nullptr, 0, &total)))
                return rc;
            if (total > cand_cap && n > 1) {             // size the chunk by this one's lists and ask again
                chunk = std::max<int64_t>(1, (int64_t)((double)n * (double)cand_cap / (double)total));
                continue;
            }
            const size_t T = (size_t)std::max<int64_t>(total, 1);
            if ((rc = bqidx.reserve(4 * T)) || (rc = beidx.reserve(4 * T))) return rc;
            if ((rc = lshkm_lsh_query_f64(h, W + u0 * d, n, nullptr, 1, bqptr.as<int64_t>(), bqidx.as<int32_t>(), total,
                                          &total)))
                return rc;
            if ((rc = launch_cv_exclude(s, bqptr.as<int64_t>(), bqidx.as<int32_t>(), n, (int32_t)q0, (int32_t)(q0 + F),
                                        bscr.as<int64_t>(), bra.as<int32_t>(), brb.as<int32_t>(), beptr.as<int64_t>(),
                                        beidx.as<int32_t>())))
                return rc;
            if ((rc = p_closest_launch(ctx, W, M, d, W + u0 * d, n, beptr.as<int64_t>(), beidx.as<int32_t>(), total, P,
                                       bnidx.as<int32_t>(), bnsim.as<double>(), bncnt.as<int32_t>())))
                return rc;
            // every user's one-element unknown list {hide_idx}; the users not
            // calculated (-1) get no prediction and are never summed
            if ((rc = launch_cv_predict(s, W, Wm, d, Wm + u0, n, n, bhptr.as<int64_t>() + u0, hide, bnidx.as<int32_t>(),
                                        bnsim.as<double>(), bncnt.as<int32_t>(), P, bpred.as<double>())))
                return rc;
            if ((rc = launch_cv_fold_sum(s, n, hide + u0, bold.as<double>() + u0, bpred.as<double>() + u0,
                                         beptr.as<int64_t>(), err_dev ? err_dev + u0 : nullptr, bsum.as<double>() + i,
                                         bcnt.as<int64_t>() + i, qb > 0)))
                return rc;
            qb += n;
        }
    }
    double ks[10];
    int64_t kc[10];
    const D2H rd[2] = {{ks, bsum.p, sizeof(ks)}, {kc, bcnt.p, sizeof(kc)}};
    if ((rc = d2h_batch(ctx, rd, 2))) return rc;
    double all_sum = 0;                              // main.cpp:428-434
    for (int i = 0; i < 10; i++) {
        if (kc[i] > 0) all_sum = all_sum + (ks[i] / (double)kc[i]);
        if (fold_sum_host) fold_sum_host[i] = ks[i];
        if (fold_cnt_host) fold_cnt_host[i] = kc[i];
    }
    *mae_host = all_sum / 10;
    return 0;
}

}  // extern "C"
