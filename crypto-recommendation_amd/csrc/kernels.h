// kernels.h — launchers of the gfx950 kernels (host-callable, stream-ordered).
#pragma once
#include <climits>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact_layout.h"
#include "fused_layout.h"
#include "recom_layout.h"

namespace lshkm {

// Dataset rows in HBM: fp32 (the storage the hot path is tuned for: the
// synthetic / proj-2 values are fp32-representable) or fp64 (general doubles,
// e.g. the recommender's user vectors, crypto_rec.hpp:78-140).
// Kernels that read rows are templated on the element type; launchers take a
// Pts and dispatch.
struct Pts {
    const void* p = nullptr;
    bool f64 = false;
    Pts() = default;
    Pts(const float* x) : p(x), f64(false) {}
    Pts(const double* x) : p(x), f64(true) {}
    const float* f() const { return static_cast<const float*>(p); }
    const double* d() const { return static_cast<const double*>(p); }
    size_t esize() const { return f64 ? 8 : 4; }
    // row r of a [.][d] matrix
    Pts row(int64_t r, int d) const {
        Pts q = *this;
        q.p = static_cast<const char*>(p) + (size_t)r * d * esize();
        return q;
    }
};
// The row-type dispatch of a launcher: f(X.d()) or f(X.f()), f a generic lambda.
template <typename F>
inline void with_rows(Pts X, F&& f) {
    if (X.f64) f(X.d());
    else f(X.f());
}

// One assignment: rows, centroids, metric and the two outputs.
struct AssignJob {
    Pts X;
    int64_t N = 0;
    int d = 0;
    const double* C = nullptr;       // [K][d]
    int K = 0;
    int metric = 0;
    int32_t* assign = nullptr;       // [N]
    double* dist = nullptr;          // [N]
};

// A list on the device as the launchers take it: int32 rows, or u64 records
// (row in the low or high half, per list). Flat (nseg == 0): entries
// [0, min(*count, bound)). Segmented (the fused kernels' lists,
// fused_layout.h): segment b = p[b * seg_rows ..], its length
// counts[SEG_SLOTS * b + slot], rows in slot SEG_ROWS and records in SEG_FIX;
// count then holds the segments' total.
// bound <= 0: nothing to launch. p == NULL (flat): every row below bound.
template <typename T>
struct DevList {
    static constexpr int slot = sizeof(T) == 4 ? SEG_ROWS : SEG_FIX;
    T* p = nullptr;
    unsigned long long* count = nullptr;
    int64_t bound = 0;
    int32_t* counts = nullptr;
    int64_t seg_rows = 0;
    int nseg = 0;
    const int32_t* seg_counts() const { return nseg > 0 ? counts : nullptr; }
};
using RowList = DevList<int32_t>;
using RecList = DevList<unsigned long long>;

// Projection families, one launcher (hash.hip).
enum HashMode {
    HM_LSH_EUCLID = 0,    // EuclideanPhiGen: tuples + phi + bucket
    HM_LSH_COSINE = 1,    // CosineGGen: g (= phi = bucket)
    HM_CUBE_EUCLID_H = 2, // EuclideanFGen's inner h values [N][k]
    HM_CUBE_COSINE = 3,   // HypercubeGen over CosineHGen: vertex [N]
};

struct HashParams {
    const double* PT;     // [d][LKpad] projections, transposed (fp32 V widened exactly, or fp64 R)
    const float* t;       // [LK]   (euclidean)
    const double* pnorm;  // [LK]   ||projection||_2, rounded up
    const int32_t* r;     // [LK]   (LSH euclidean)
    float w;
    int d, L, k, LK, LKpad;
    int64_t nb;
};
int hash_fb(int LK);      // projections per accumulator block
int hash_lkpad(int LK);   // padded PT row length

int launch_proj_hash(hipStream_t s, int mode, Pts X, int64_t N, const HashParams& p,
                     int32_t* out_h, int32_t* out_phi, int32_t* out_bucket,
                     unsigned long long* stats);

// Split-f16 MFMA hashing (hash_mfma.hip): fp32 points, d = 128, L*k <= 32.
struct HashMfmaParams {
    const _Float16* Vh;   // [>= 32][128] f16 hi of the projections (rows >= LK zero)
    const _Float16* Vl;   // lo
    const float* t;       // [LK] (euclidean)
    const double* pnorm;  // [LK] |v|_2 rounded up
    const double* v1;     // [LK] |v|_1 rounded up
    const int32_t* r;     // [LK] (LSH euclidean)
    const double* PT;     // [d][LKpad] fp64 projections (the fix-up pass)
    float w;
    int d, L, k, LK, LKpad;
    int64_t nb;
};
// out_h: LSH euclidean tuples [N][L*k] / cube euclidean h [N][k] / cube cosine
// vertex [N]; mm: cube euclidean h range (atomicMin/Max into a pre-set pair).
// list: the workspace for the uncertified rows (p, counts, bound = the entries
// p holds); the launch splits it in per-block segments (hash_mfma_seg_rows).
int launch_hash_mfma(hipStream_t s, int mode, const float* X, int64_t N, const HashMfmaParams& p, int32_t* out_h,
                     int32_t* out_phi, int32_t* out_bucket, int32_t* mm, const RecList& list,
                     unsigned long long* stats, int h16 = 0);

// Lloyd assignment (assign.hip).
int assign_dp(int d);    // padded dimension used by the MFMA kernel (0 = unsupported)
int launch_centroid_prep(hipStream_t s, const double* C, int K, int Kpad, int d, int DP, int metric, bool xf64,
                         float* C32, float* cconst);
int launch_assign_mfma(hipStream_t s, Pts X, int64_t N, int d, int DP, const double* C, int K,
                       int Kpad, int metric, const float* C32, const float* cconst, int32_t* assign, double* dist,
                       int32_t* ambig, unsigned long long* ambig_count);
// Lloyd cosine winners whose distance the certified form declined (list at
// rows[0..*count), written by assign_mfma_kernel<., 1>): soft-x87 distances.
int launch_cos_fix(hipStream_t s, Pts X, int64_t N, int d, const double* C, const int32_t* rows,
                   const unsigned long long* count, const int32_t* assign, double* dist);
// The exact pass (exact_pass.hip) over the rows of l in the given form
// (exact_route, exact_layout.h); ws: exact_ws_bytes(form, d, K) bytes that
// launch_exact_prep filled for these centroids on this stream (the form's
// centroid-only part: it may run ahead of the pass that fills l).
// exact_dist false (LSHKM_DIST_CERTIFIED; the pruned forms, euclidean): a winner
// distance may come from the x*x chain (<= 2^-44 relative); cluster IDs are the
// reference's either way. xn2 / nbv (every, cosine): the rows' and centroids'
// sums of squares, where the caller has them.
int launch_exact_prep(hipStream_t s, const AssignJob& q, ExactForm form, void* ws);
int launch_exact_pass(hipStream_t s, const AssignJob& q, const RowList& l, ExactForm form, const void* ws,
                      bool exact_dist, const double* xn2, const double* nbv);
int launch_assign_override(hipStream_t s, const int32_t* src_rows, int K, int64_t N, int32_t* assign,
                           double* dist);

int launch_add_counter(hipStream_t s, unsigned long long* dst, const unsigned long long* src);
// stats[dst_idx[i]] += *src[i], i < n <= 8, in one launch
int launch_add_counters(hipStream_t s, unsigned long long* stats, int n, const int* dst_idx,
                        const unsigned long long* const* src);
// The fused assignment's last kernel: stats[dst_idx[i]] += *srcs[i] (i < n <= 8),
// then cnt[0, ncnt) and cb[0, ncb) zeroed, and the centroid override of
// src_rows (device) where it is not NULL (K > 8192: by launch_assign_override
// after it).
int launch_fused_epilogue(hipStream_t s, unsigned long long* stats, int n, const int* dst_idx,
                          const unsigned long long* const* srcs, unsigned long long* cnt, int ncnt, unsigned int* cb,
                          int ncb, const int32_t* src_rows, int K, int64_t N, int32_t* assign, double* dist);

// Stable bucket scatter (scatter.hip).
size_t sort_scratch_bytes(int64_t N, int64_t range, int T = 1);
// Distinct int32 keys, n <= 8192: one-workgroup bitonic sort of (key, val) pairs.
// n_dev: the count is read on the device instead; n is then the caller's bound on
// it (refused past 8192).
// The pow contract (pow2.hip): lshkm_pow_selfcheck once per process; 0, or
// LSHKM_ERR_UNSUPPORTED with the error set when this process's pow differs.
int pow_contract_check();

int sort_pairs_small(hipStream_t s, const int32_t* keys, const int32_t* vals, int64_t n, int32_t* keys_out,
                     int32_t* vals_out, const unsigned int* n_dev = nullptr);
int stable_sort_by_key(hipStream_t s, const int32_t* keys, int64_t kstride, const int32_t* vals, int64_t N,
                       int64_t range, int32_t* keys_out, int32_t* vals_out, void* scratch);
int launch_csr_bounds(hipStream_t s, const int32_t* sorted_keys, int64_t N, int64_t nb, int64_t* row_ptr, int T = 1);
// T independent stable sorts in one set of launches (table t: keys + t * key_ts,
// vals + t * val_ts; outputs at + t * N).
int stable_sort_by_key_batched(hipStream_t s, const int32_t* keys, int64_t kstride, int64_t key_ts, const int32_t* vals,
                               int64_t val_ts, int T, int64_t N, int64_t range, int32_t* keys_out, int32_t* vals_out,
                               void* scratch);

// Queries (query.hip).
size_t scan_ws_bytes(int64_t M);
int launch_scan_i64(hipStream_t s, const int64_t* a, int64_t M, int64_t* out, int64_t* scratch = nullptr);
int launch_lsh_query(hipStream_t s, const int32_t* qbucket, const int32_t* qtuple, const int32_t* alias, int64_t nq,
                     int L, int k, int64_t nb, int filtered, int64_t N, const int32_t* tuples, const int32_t* bucket,
                     const int64_t* row_ptr, const int32_t* idx, int64_t* sizes, int64_t* cand_off,
                     int32_t* klist, int64_t* kcount, int64_t* qsz, int64_t* out_ptr, int32_t* out, int phase,
                     int64_t* scan_ws = nullptr, const int32_t* mt0 = nullptr);
int launch_lsh_gather_t0(hipStream_t s, const int32_t* tuples, const int32_t* idx, int64_t N, int L, int k, int32_t* mt0);
int launch_cube_query(hipStream_t s, const int32_t* qvert, int64_t nq, const int32_t* masks, int S,
                      const int64_t* row_ptr, const int32_t* idx, int64_t* sizes, int64_t* slot_off,
                      int64_t* out_ptr, int32_t* out, int64_t* scan_ws = nullptr);

// Hypercube coins (cube.hip).
int launch_h_minmax(hipStream_t s, const int32_t* h, int64_t n, int32_t* mm_dev);
// h: int32 [N][k], or int16 when h16 (the hash kernel's narrow output).
int launch_coin_first(hipStream_t s, const void* h, bool h16, int64_t N, int k, int32_t hmin, int32_t hspan,
                      const int32_t* memo, int32_t* first_row);
int launch_coin_collect(hipStream_t s, int32_t* first_row, int64_t total, int k, int32_t hspan, int32_t* keys,
                        int32_t* vals, unsigned int* count);
int launch_coin_draw(hipStream_t s, const int32_t* sorted_vals, const unsigned int* count, int32_t hmin, int32_t hspan,
                     int32_t* memo, uint32_t* state);
int launch_coin_vertex(hipStream_t s, const void* h, bool h16, int64_t N, int k, int32_t hmin, int32_t hspan,
                       const int32_t* memo, int32_t* vertex);
int launch_memo_rehome(hipStream_t s, const int32_t* old_memo, int32_t old_min, int32_t old_span, int32_t* new_memo,
                       int32_t new_min, int32_t new_span, int k);
int launch_memo_scatter(hipStream_t s, const int32_t* off, const int32_t* bit, int64_t n, int32_t* memo);

// k-means update (update.hip).
// The sequential chains. carry / carry_counts (may be NULL): the running sums
// and counts the chain continues from (exact-order sharded mode); flag != NULL:
// only the flagged (cluster, 64-dim block) chains.
int launch_km_chain(hipStream_t s, Pts X, int d, const int32_t* rows, const int64_t* crow, int K,
                    double* sums, int64_t* counts, const double* carry = nullptr,
                    const int64_t* carry_counts = nullptr, const int* flag = nullptr);
// The same sums by binade segments (kmseg.h; ws: km_seg_ws_bytes): every chain
// of fp64 rows; flag != NULL: only the flagged (cluster, 64-dim block) chains.
size_t km_seg_ws_bytes(int64_t M, int K, int d);
// above this the update takes the fixed-point form instead (same exact sums)
constexpr size_t KM_SEG_WS_CAP = (size_t)8 << 30;
int launch_km_sums_seg(hipStream_t s, Pts X, int d, const int32_t* rows, const int64_t* crow, int K, int64_t M,
                       double* sums, int64_t* counts, const double* carry, const int64_t* carry_counts, void* ws,
                       const int* flag = nullptr);
// Same sums, parallel: plain fp64 adds in any order wherever the sequential
// chain provably never rounds (km_cert), the rounding chains by segments
// (seg_ws: km_seg_ws_bytes) or, without seg_ws, by the sequential kernel
// (ws: km_fx_ws_bytes). stat: counts the chains the test flags.
size_t km_fx_ws_bytes(int K, int d);
int launch_km_sums_fx(hipStream_t s, Pts X, int d, const int32_t* rows, const int64_t* crow, int K, int64_t M,
                      double* sums, int64_t* counts, const double* carry, const int64_t* carry_counts, void* ws,
                      unsigned long long* stat = nullptr, void* seg_ws = nullptr);
// Sharded form (lshkm_kmeans_shard_*): begin (ws: km_fx_ws_bytes), certify,
// prepare / chain (the flagged chains' records and their composition; ws:
// km_shard_ws_bytes).
size_t km_shard_ws_bytes(int64_t M, int K, int d);
int launch_km_shard_begin(hipStream_t s, Pts X, int d, const int32_t* rows, const int64_t* crow, int K, int64_t M,
                          double* sums, double* asum, int32_t* qt, int64_t* counts, void* ws);
int launch_km_shard_certify(hipStream_t s, const double* gathered, int world, int rank, const double* asum,
                            const int32_t* qt, const int64_t* counts, int K, int d, double* sums_out, double* start,
                            int* flag, uint8_t* mask, unsigned long long* nflag);
int launch_km_shard_prepare(hipStream_t s, Pts X, int d, const int32_t* rows, const int64_t* crow, int K, int64_t M,
                            const double* start, const int* flag, const uint8_t* mask, void* ws);
int launch_km_shard_chain(hipStream_t s, Pts X, int d, const int32_t* rows, const int64_t* crow, int K, int64_t M,
                          const int* flag, const uint8_t* mask, const double* carry, void* ws, double* sums);
// Column chains of K row blocks [crow[k], crow[k+1]) of a row-major [n][m]
// fp64 matrix (row order, from carry [K][m] or 0; iota from launch_seg_iota;
// ws: seg_columns_ws_bytes) by binade segments -> out [K][m].
size_t seg_columns_ws_bytes(int64_t n, int K, int m);
int launch_seg_iota(hipStream_t s, int32_t* iota, int64_t n);
int launch_seg_columns(hipStream_t s, const double* V, int64_t n, int K, int m, const int32_t* iota,
                       const int64_t* crow, const double* carry, double* out, void* ws);
// Grid test of a matrix's values (update.hip): qt [3] device ints; after the
// copy back, grid_exact_squares says whether every difference of two values
// squares exactly with pow(x, 2) == x*x.
int launch_grid_bits(hipStream_t s, Pts X, int64_t n, int* qt);
bool grid_exact_squares(const int* qt_host);
int launch_km_finalize(hipStream_t s, const double* sums, const int64_t* counts, int K, int d, const double* C_old,
                       int metric, double min_dist, double* C_new, int* moved);

// k-means++ seeding (kmeanspp.hip): iterations 1..K-1 on the stream.
// chosen[0] and canon[1..K-1] (the engine's canonical draws) already on the
// device; ws holds kpp_layout(N).bytes bytes (kpp_layout.h).
int launch_kmeans_pp(hipStream_t s, Pts X, int64_t N, int d, int K, int metric, const double* canon,
                     int32_t* chosen, void* ws, unsigned long long* stats);
// One iteration over a row shard of n >= 1 rows (lshkm_kpp_shard_*), the host
// between the steps; ws as above for n rows. Each step leaves what the host
// reads in the KppShardOut at ws + kpp_layout(n).out (kpp_layout.h). crow: the
// newest centroid's [d] row, of X's type.
int launch_kpp_shard_dist(hipStream_t s, Pts X, int64_t n, int d, int metric, const void* crow, int it, void* ws);
int launch_kpp_shard_units(hipStream_t s, int64_t n, unsigned long long gmax_bits, double start, void* ws);
int launch_kpp_shard_chain(hipStream_t s, int64_t n, double s_in, void* ws, unsigned long long* stats);
int launch_kpp_shard_pick(hipStream_t s, int64_t n, double rd, int owns_row0, void* ws);

// Recommend step (recom.hip): fp64 rows, per-user candidate CSR.
int launch_rc_norms(hipStream_t s, const double* X, int64_t N, int d, double* xa);
// The clustering recommender (lshkm_cluster_*): recom_layout.h states its form
// rule and workspaces. One call's inputs: rows X [N][d] with their means, the
// cluster CSR (crow [K + 1], crows), the users U [nq][d] with their means and
// clusters, the unknown-index CSR.
struct RecomJob {
    Pts X;
    const double* x_mean;
    int64_t N;
    int d;
    const int64_t* crow;
    const int32_t* crows;
    int K;
    Pts U;
    const double* u_mean;
    int64_t nq;
    const int32_t* ucl;
    const int64_t* unk_ptr;
    const int32_t* unk_idx;
};
// The running prediction sums between shards: main [total unknowns], abs / cnt
// [nq]. As the carry in (only read; all NULL on the first shard) and as the
// carry out (all NULL on the final step, which writes RecomOut instead).
struct RecomCarry {
    double *main, *abs;
    int64_t* cnt;
};
// The final step: predictions (pred / pidx [total unknowns], workspace), then
// out [nq][n_top]. All NULL when the running sums are carried on.
struct RecomOut {
    double* pred;
    int32_t* pidx;
    int n_top;
    int32_t* out;
};
// one wave per user (rows of any size): scratch = rc_wave_scratch(nq, largest cluster)
int launch_rc_cluster_top_n(hipStream_t s, const RecomJob& j, double* scratch, const RcWaveScratch& ws,
                            const RecomOut& o, unsigned long long* soft_count);
// The terms form (recom_route): similarities and the per-(member, unknown index)
// terms of every user at once, then the chains one wave per user (its chains
// lane by lane), then the quicksort per user.
struct RcGroups {                // the device image of RcWorkList / RcPackLayout
    const int32_t* ioff;
    int ngroups;
    int64_t nitems;
    const int32_t* gcl;
    const int32_t* gptr;
    const int32_t* gusr;
    void* items;              // nitems x RC_ITEM_BYTES
    int64_t nusers;
    void* users;              // nusers x RC_USER_BYTES
};
struct RcTermsOut {              // soff / toff [nq + 1] on the device, total = soff[nq]
    const int64_t *soff, *toff;
    int64_t total;
    double *sims, *terms;
};
// map: the base of a buffer of rc_map_layout(total, nq)
int launch_rc_terms(hipStream_t s, const RecomJob& j, const RcTermsOut& t, char* map, const RcGroups& groups,
                    unsigned long long* soft_count);
struct RcLong {                  // one batch of long users (RcLongBatch) in its RcLongLayout
    const RcLongUser* tab;
    int64_t nlong, rows;
    int D;
    const int64_t* crow;
    double *V, *carry, *sums;
    int32_t* iota;
    void* ws;
};
// users of fewer than long_min members (INT64_MAX: every user)
int launch_rc_chain_terms(hipStream_t s, const RecomJob& j, const RcTermsOut& t, const RecomCarry& in,
                          const RecomCarry& out, double* pred, int64_t long_min);
int launch_rc_long(hipStream_t s, const RcTermsOut& t, const RecomCarry& in, const double* u_mean,
                   const RecomCarry& out, double* pred, const RcLong& lng);
int launch_rc_top(hipStream_t s, const RecomJob& j, const int64_t* soff, const int64_t* carry_cnt, const RecomOut& o);
int launch_rc_shard_sims(hipStream_t s, const RecomJob& j, const int64_t* soff, double* sims,
                         unsigned long long* soft_count);
int launch_rc_shard_chain(hipStream_t s, const RecomJob& j, const int64_t* soff, const double* sims,
                          const RecomCarry& in, const RecomCarry& out, const RecomOut& o);
int launch_rc_p_closest(hipStream_t s, const double* X, const double* xa, int d, const double* U, int64_t nq,
                        const int64_t* cand_ptr, const int32_t* cand_idx, int P, double* sim, double* key,
                        int32_t* pos, int32_t* out_idx, double* out_sim, int32_t* out_cnt, int32_t* replay,
                        unsigned int* replay_count, bool replay_pass = true);
int launch_rc_top_n(hipStream_t s, const double* X, const double* x_mean, int d, const double* u_mean, int64_t nq,
                    const int64_t* unk_ptr, const int32_t* unk_idx, const int32_t* nb_idx, const double* nb_sim,
                    const int32_t* nb_cnt, int P, int n_top, double* pred, int32_t* pidx, int32_t* out);

// 10-fold validation of the LSH recommender (crossval.hip; main.cpp:393-437).
// rows (may be NULL = identity): user m is row rows[m] of X and of the
// unknown-index CSR.
int launch_cv_gather(hipStream_t s, const double* X, const double* x_mean, const int32_t* rows, int64_t M, int d,
                     double* W, double* w_mean);
int launch_cv_hide(hipStream_t s, const double* X, const double* x_mean, const int32_t* rows, int64_t M, int d,
                   const int64_t* unk_ptr, const int32_t* unk_idx, const int32_t* draw, double* H, double* h_mean,
                   int32_t* hide_idx, double* old);
int launch_cv_exclude(hipStream_t s, const int64_t* in_ptr, const int32_t* in_idx, int64_t nq, int32_t lo, int32_t hi,
                      int64_t* cnt, int32_t* run_a, int32_t* run_b, int64_t* out_ptr, int32_t* out_idx);
int launch_cv_predict(hipStream_t s, const double* X, const double* x_mean, int d, const double* u_mean, int64_t nq,
                      int64_t entries, const int64_t* unk_ptr, const int32_t* unk_idx, const int32_t* nb_idx,
                      const double* nb_sim, const int32_t* nb_cnt, int P, double* pred);
int launch_cv_fold_sum(hipStream_t s, int64_t F, const int32_t* hide_idx, const double* old, const double* pred,
                       const int64_t* nb_ptr, double* err, double* k_sum_out, int64_t* cnt_out, bool carry);

// Range assignment (range.hip).
int launch_range_radius(hipStream_t s, const double* C, int K, int d, int metric, double* r0,
                        unsigned long long* tmp);
int launch_range_pairs(hipStream_t s, const int64_t* comb_ptr, const int32_t* comb_idx, int K, int32_t* rows,
                       int32_t* cents);
int launch_range_init(hipStream_t s, int64_t N, int32_t* assign, double* dist);
int launch_range_pass(hipStream_t s, Pts X, int d, const double* C, int K, int metric, const int32_t* key,
                      const int64_t* vptr, const int32_t* cents, double* cache, int8_t* cached, int64_t N,
                      const double* r0, int64_t pass, int32_t* assign, double* dist, unsigned long long* count);
int launch_range_unassigned(hipStream_t s, const int32_t* assign, int64_t N, int32_t* list,
                            unsigned long long* count);
// Xr: rows of the same element type as X
int launch_range_gather(hipStream_t s, Pts X, int d, const int32_t* list, int64_t M, void* Xr);
int launch_range_scatter(hipStream_t s, const int32_t* list, int64_t M, const int32_t* ar, const double* dr,
                         int32_t* assign, double* dist);

// Silhouette (silhouette.hip).
int launch_sil_near(hipStream_t s, const double* C, int K, int d, int metric, int32_t* near);
int launch_sil_points(hipStream_t s, Pts X, int d, int metric, const int32_t* rows, const int64_t* crow,
                      const int32_t* assign, const int32_t* near, int64_t N, double* s_out, bool exsq = false);
int launch_sil_sum(hipStream_t s, const double* sv, const int32_t* rows, const int64_t* crow, int K, int64_t N,
                   double* raw, double* out);

// PAM medoid update (pam.hip). Positions q index the cluster CSR (rows[q]).
// bad [1]: set when an assign value lies outside [0, K).
int launch_pam_check_assign(hipStream_t s, const int32_t* assign, int64_t N, int K, int* bad);
// The screen (euclidean, d <= PAM_SCREEN_DMAX): per position the f32-rounded
// row's |x|^2 (n2) and |x - f32(x)| rounded up (rho); cbad[c] != 0 when cluster
// c holds a row outside the range the bound assumes (non-finite, |x| >= 2^50);
// cmax[c] (zeroed by the caller): the bits of the cluster's largest n2.
constexpr int PAM_SCREEN_DMAX = 128;
constexpr int PAM_SCREEN_COLS = 128;     // members owned by one block of the screen
int launch_pam_prep(hipStream_t s, Pts X, int d, const int32_t* rows, const int32_t* assign, int64_t N, double* n2,
                    float* rho, int* cbad, unsigned long long* cmax);
// items [nitems]: (cluster, first owned member) of every block; per member of
// a screened cluster the approximate dist_sum and its bound in two parts:
// St / Et [N] from the tiles it owned a column of, Sfix / Efix [N] (zeroed by
// the caller; fixed point) from the tiles it was a row of.
int launch_pam_screen(hipStream_t s, Pts X, int d, const int32_t* rows, const int64_t* crow, const int2* items,
                      int64_t nitems, const double* n2, const float* rho, double* St, double* Et,
                      const unsigned long long* cmax, unsigned long long* Sfix, unsigned long long* Efix);
// screen [K] (host's choice per cluster) + cbad -> flag [N] (1 = the member goes
// to the exact chain), cnt [K]; stats: the context's counters.
int launch_pam_mark(hipStream_t s, const int64_t* crow, int K, const int32_t* screen, const int* cbad,
                    const double* St, const double* Et, const unsigned long long* cmax,
                    const unsigned long long* Sfix, const unsigned long long* Efix, uint8_t* flag, int64_t* cnt,
                    unsigned long long* stats);
// coff [K + 1] = scan of cnt: cand [coff[K]] = the flagged positions in order.
int launch_pam_compact(hipStream_t s, const int64_t* crow, int K, const uint8_t* flag, const int64_t* coff,
                       int32_t* cand);
// sums[i] = dist_sum of candidate i (position cand[i], or i when cand is NULL;
// m_dev: the candidate count on the device, NULL = N), in exact.h's order.
int launch_pam_exact(hipStream_t s, Pts X, int d, int metric, const int32_t* rows, const int64_t* crow,
                     const int32_t* assign, const int32_t* cand, const int64_t* m_dev, int64_t N, double* sums,
                     bool exsq);
// The reference's selection over each cluster's candidates [coff[c], coff[c+1])
// (coff = crow when cand is NULL): med [K] = the medoid's row (-1: empty
// cluster), csum [K] its dist_sum (-1.0: empty).
int launch_pam_select(hipStream_t s, const int32_t* rows, const int32_t* cand, const int64_t* coff, int K,
                      const double* sums, int32_t* med, double* csum);
// C_new[c] = row med[c] widened to fp64, or C_old[c] for an empty cluster.
int launch_pam_gather(hipStream_t s, Pts X, int d, const int32_t* med, int K, const double* C_old, double* C_new);

// lshkm_lsh_p_closest's screen (lsh_closest.hip; lshpc_layout.h states the
// routing rule and the workspaces). One side's f32 image: x^ [n][dp], the
// packed bucket codes, 1 / |x^| (negative: poison), the bound's conversion term.
struct LshpcSide {
    const float* xh;
    const uint32_t* code;
    const float* inv;
    const float* rel;
    int64_t n;
};
// The kept-lists of one chunk of users: (lo, hi, row) [segs][np][cap] and the
// states [4][segs][np] (count, candidates seen, T's bits, flag).
struct LshpcKept {
    float *klo, *khi;
    int32_t *krow, *state;
    int64_t np, seg_rows;
    int cap, segs;
};
int launch_lshpc_prep(hipStream_t s, const double* X, int64_t n, int d, int dp, const double* xa, const int32_t* bucket,
                      int L, int k, const LshpcSide& out);
int launch_lshpc_screen(hipStream_t s, int dp, const LshpcSide& rows, const LshpcSide& users, int32_t excl_lo,
                        int32_t excl_hi, int P, int L, int k, const LshpcKept& kept);
// The same screen over hypercube vertices (codes = vertices, no exclusion):
// candidates by cubepc_member(code_i ^ code_j, probe).
struct CubeProbe;
int launch_cubepc_screen(hipStream_t s, int dp, const LshpcSide& rows, const LshpcSide& users, int P,
                         const CubeProbe& probe, const LshpcKept& kept);
// The cube's lists path: vg[i] = vertex[list[i]], ncand[i] = the length of that
// user's combined bucket over the S probe masks.
int launch_cubepc_handed(hipStream_t s, const int32_t* vertex, const int32_t* list, int64_t m, const int32_t* masks,
                         int S, const int64_t* row_ptr, int32_t* vg, int64_t* ncand);
// The segments joined: nkept [n], ncand [n] (or NULL), cptr [n + 1] = scan of
// nkept, cidx = the unflagged users' kept rows, ascending; stats 14 / 15.
int launch_lshpc_join(hipStream_t s, const LshpcKept& kept, int64_t n, int P, int64_t* nkept, int64_t* ncand,
                      int64_t* cptr, int32_t* cidx, unsigned long long* stats);
// handed += u0 + the chunk's flagged users and the settle's replay list.
int launch_lshpc_collect(hipStream_t s, const LshpcKept& kept, int64_t n, int64_t u0, const int32_t* replay,
                         const unsigned int* replay_count, int32_t* handed, unsigned int* handed_count);
int launch_lshpc_stats(hipStream_t s, unsigned long long* stats, int64_t settled, int64_t lists);
int launch_lshpc_gather(hipStream_t s, const double* U, int d, const int32_t* list, int64_t m, double* Ug);
int launch_lshpc_scatter(hipStream_t s, const int32_t* list, int64_t m, int P, const int32_t* gidx, const double* gsim,
                         const int32_t* gcnt, const int64_t* eptr, int32_t* out_idx, double* out_sim, int32_t* out_cnt,
                         int64_t* ncand);

// lshkm_min_vector_dist (nearest.hip; nearest_layout.h states the routing rule
// and the workspace). One side's f32 image: x^ [n][dp], a (|x^|^2 euclidean,
// 1 / |x^| cosine; negative: poison), the bound's conversion term.
struct NearestSide {
    const float* xh;
    const float* a;
    const float* rel;
    int64_t n;
};
// The screen's state per query: the smallest hi's key, the count of rows with
// lo <= it, the first cap of them.
struct NearestKept {
    uint32_t* minkey;
    int32_t *cnt, *krow;
    int64_t seg_rows;
    int cap;
};
// pois / npois (rows; NULL for the queries): the poison rows' list and count.
int launch_nearest_prep(hipStream_t s, Pts X, int64_t n, int d, int dp, int metric, const NearestSide& out, int32_t* pois,
                        unsigned int* npois);
// Both passes over a grid of tiles x segs blocks.
int launch_nearest_screen(hipStream_t s, int dp, int metric, const NearestSide& rows, const NearestSide& qs,
                          const NearestKept& kept, int64_t tiles, int segs);
// ptr != NULL: the lists form over idx[ptr[q] .. ptr[q+1]) (first in list wins
// ties); else the kept rows and the poison rows of the queries the screen did
// not flag. stats 19 += the distances computed.
int launch_nearest_settle(hipStream_t s, Pts X, Pts Q, int64_t nq, int d, int metric, const int64_t* ptr,
                          const int32_t* idx, const NearestKept& kept, const float* qa, const int32_t* pois,
                          const unsigned int* npois, const double* xn2, const double* qn2, double* dist, int32_t* row,
                          unsigned long long* stats);
// list += the flagged queries (a poison query, more than cap rows); stats 17 / 18.
int launch_nearest_collect(hipStream_t s, const NearestKept& kept, const float* qa, int64_t nq, int32_t* list,
                           unsigned int* count, unsigned long long* stats);
// All N rows for the queries of list[0 .. *count) (list NULL: all nq, stats 18 += nq).
int launch_nearest_scan(hipStream_t s, Pts X, int64_t N, Pts Q, int64_t nq, int d, int metric, const int32_t* list,
                        const unsigned int* count, const double* xn2, const double* qn2, double* dist, int32_t* row,
                        unsigned long long* stats);
// xn2 / qn2 of the two launchers above: the rows' / queries' sequential sums of
// squares (launch_rc_norms), read for cosine on fp64 values only.
bool nearest_needs_norms(Pts X, int metric);
int launch_nearest_norms(hipStream_t s, Pts X, int64_t n, int d, int metric, double* xa);
int launch_nearest_empty(hipStream_t s, int64_t nq, double* dist, int32_t* row);
// *bad = 1 on a ptr that does not start at 0 or decreases, or an idx outside [0, N).
int launch_nearest_check(hipStream_t s, const int64_t* ptr, int64_t nq, const int32_t* idx, int64_t total, int64_t N,
                         unsigned int* bad);

// lshkm_knn (knn.hip; knn_layout.h states the routing rule and the workspace).
// The screen's state per query: its (query, group) keys, the k-th smallest of
// them, the count of rows with lo <= it, the first cap of them. The images,
// the prep, the norms and the lists check are lshkm_min_vector_dist's.
struct KnnKept {
    uint32_t *gkey, *tau;
    int32_t *cnt, *krow;
    int64_t seg_rows;
    int groups, grp_shift, cap, k;
};
// Pass 1, the select and pass 2 over a grid of tiles x segs blocks.
int launch_knn_screen(hipStream_t s, int dp, int metric, const NearestSide& rows, const NearestSide& qs,
                      const KnnKept& kept, int64_t tiles, int segs);
// ptr != NULL: the lists form over idx[ptr[q] .. ptr[q+1]) (key = the position);
// else the kept rows and the poison rows of the queries the screen did not
// hand over. row / dist [nq][k], cnt [nq] or NULL. stats 22 += the distances computed.
int launch_knn_settle(hipStream_t s, Pts X, Pts Q, int64_t nq, int d, int metric, int k, const int64_t* ptr,
                      const int32_t* idx, const KnnKept& kept, const float* qa, const int32_t* pois,
                      const unsigned int* npois, const double* xn2, const double* qn2, int32_t* row, double* dist,
                      int32_t* cnt, unsigned long long* stats);
// list += the handed queries (a poison query, no threshold, more than cap rows); stats 20 / 21.
int launch_knn_collect(hipStream_t s, const KnnKept& kept, const float* qa, int64_t nq, int32_t* list,
                       unsigned int* count, unsigned long long* stats);
// All N rows for the queries of list[0 .. *count) (list NULL: all nq, stats 21 += nq).
int launch_knn_scan(hipStream_t s, Pts X, int64_t N, Pts Q, int64_t nq, int d, int metric, int k, const int32_t* list,
                    const unsigned int* count, const double* xn2, const double* qn2, int32_t* row, double* dist,
                    int32_t* cnt, unsigned long long* stats);
int launch_knn_empty(hipStream_t s, int64_t nq, int k, int32_t* row, double* dist, int32_t* cnt);

// User vectors from scored tweets (uservec.hip). The visit list and the tweet
// table of one lshkm_user_sums call: visit v = tweet tw[v] onto group grp[v]
// (-1: skipped), tweet t's score and its coins ci_idx[ci_ptr[t] .. ci_ptr[t+1]).
struct UvVisits {
    const int32_t *tw, *grp;
    int64_t V;
    const double* score;
    const int64_t* ci_ptr;
    const int32_t* ci_idx;
    int64_t T, G;
    int C;
};
// *flag |= 1 (tw), 2 (grp), 8 (ci_ptr) with coins = false; 4 (ci_idx) with
// coins = true, which reads ci_idx through ci_ptr and so runs after the first passed.
int launch_uv_check(hipStream_t s, const UvVisits& q, bool coins, uint32_t* flag);
int launch_uv_count(hipStream_t s, const UvVisits& q, int64_t* cnt);
size_t uv_sort_bytes(int64_t E, int64_t nkeys);
int launch_uv_sums(hipStream_t s, const UvVisits& q, const int64_t* off, int64_t E, const double* carry_sum,
                   const uint8_t* carry_known, int32_t* keys, int32_t* vals, int32_t* keys_s, int32_t* vals_s,
                   void* sort_ws, int64_t* row_ptr, int32_t* long_list, uint32_t* long_count, double* sum,
                   uint8_t* known);
int launch_uv_finish(hipStream_t s, const double* sum, const uint8_t* known, int64_t G, int C, int64_t* kept,
                     int64_t* nunk, int64_t* row_off, int64_t* unk_off, double* mean, int64_t* scan_ws, double* U,
                     double* mean_out, int64_t* unk_ptr, int32_t* unk_idx, int32_t* src);

// Synthetic data.
int launch_synth(hipStream_t s, uint64_t seed, int64_t row0, int64_t rows, int d, float* X, int kind = 0);

}  // namespace lshkm
