/*
 * lshkm.h — C ABI of the MI355X (gfx950) LSH / hypercube / k-means hot path.
 *
 * Drop-in boundary for the reference's header-template interface
 * (paths relative to the reference root):
 *   create_LSH_hashtables            lib/lsh_cube.hpp:44-74
 *   get_LSH_combined_buckets         lib/lsh_cube.hpp:77-90
 *   get_LSH_filtered_combined_buckets lib/lsh_cube.hpp:93-106
 *   create_hypercube                 lib/lsh_cube.hpp:108-136
 *   get_hypercube_combined_buckets   lib/lsh_cube.hpp:139-177
 *   lloyds_assignment                lib/clustering_phases/assignment.hpp:54-80
 *   k_means                          lib/clustering_phases/update.hpp:37-86
 *   lsh_/cube_range_assignment       lib/clustering_phases/assignment.hpp:108-217
 *   silhouette_cluster               lib/clustering_phases/silhouette.hpp:31-144
 *   VectorReader<double>::read       lib/in_out/vector_reader.hpp:54-85
 *   file_to_args + ArgParser, get_config  lib/utils.cpp:53-69, lib/in_out/arg_parser.cpp, main.cpp:512-554
 *   HashGenerator plugin ABI         lib/generators/hash_generator.hpp:19-31
 *   CustHashtable::getBucketFromIndex / getHash lib/data_structures/cust_hashtable.hpp:116-125
 *
 * Conventions
 *   - Every function returns 0 on success or a negative LSHKM_ERR_* code;
 *     lshkm_last_error() then describes it (thread-local).
 *   - "_dev" pointers are device (HBM) pointers, "_host" pointers host memory.
 *     Sizes are explicit. Device outputs are written asynchronously on the
 *     context's stream; call lshkm_ctx_sync() before reading them on the host.
 *   - Points are N x d row-major rows of fp32 (the synthetic / proj-2 values
 *     are fp32-representable: the tuned storage) or of fp64: every entry
 *     point that reads dataset rows has a `_f64` twin taking `const double*`
 *     rows with the same results contract (the reference's CustVector<double>
 *     holds general doubles, e.g. the recommender's user vectors,
 *     crypto_rec.hpp:78-140). Centroids are fp64 rows, K x d.
 *   - Bit-exact with the reference: tuples, phi, bucket IDs, bucket member
 *     order, query results, hypercube vertices, probe order, cluster IDs,
 *     k-means centers and counts, chosen k-means++ rows, recommendations.
 *   - Distances (the `dist` output of the Lloyd / hash+assign entry points)
 *     follow the context's distance mode (lshkm_ctx_set_dist_mode):
 *       LSHKM_DIST_CERTIFIED (the default): euclidean winner distances may come
 *         from a certified f32 evaluation, within 2^-20 relative of the
 *         reference's fp64 value (the north star's tolerance is 1e-5); a row
 *         whose bound fails gets the reference-order chain. Zero, inf and NaN
 *         distances are reproduced bit for bit. Cluster IDs are unaffected.
 *       LSHKM_DIST_EXACT: every distance is the reference's sequential fp64
 *         chain sqrt(sum_j pow(x_j - c_j, 2)), j ascending, bit for bit --
 *         for dataset-row centroids and for general fp64 centroids after an
 *         update alike.
 *     Cosine distances, range-assignment distances, silhouettes, similarities
 *     and every other output are exact-order in both modes.
 *   - Every square the reference takes is glibc's pow(x, 2) (cust_vector.hpp:
 *     132, 149-150, 168-169), which is not x*x for ~0.085 % of general doubles
 *     (and for many exact ties): the device evaluates glibc 2.35's own
 *     algorithm (the x86-64 __pow_fma variant, csrc/gpow2.h) wherever x*x is
 *     not provably the same value. lshkm_pow_selfcheck() compares that
 *     restatement with the running process's pow; lshkm_ctx_create runs it
 *     once per process and refuses (LSHKM_ERR_UNSUPPORTED, see
 *     lshkm_last_error) on a host whose pow differs, since the reference's
 *     own results on that host could not be reproduced bit for bit.
 *   - One handle per thread; calls on a handle are serialised on its stream.
 */
#ifndef LSHKM_H
#define LSHKM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSHKM_OK 0
#define LSHKM_ERR_ARG (-1)
#define LSHKM_ERR_HIP (-2)
#define LSHKM_ERR_NOMEM (-3)
#define LSHKM_ERR_UNSUPPORTED (-4)
#define LSHKM_ERR_STATE (-5)

#define LSHKM_METRIC_EUCLIDEAN 0
#define LSHKM_METRIC_COSINE 1

#define LSHKM_DIST_CERTIFIED 0   /* euclidean winner distances within 2^-20 relative (default) */
#define LSHKM_DIST_EXACT 1       /* the reference's fp64 chain for every distance */

typedef struct lshkm_ctx_s* lshkm_ctx;
typedef struct lshkm_lsh_s* lshkm_lsh;
typedef struct lshkm_cube_s* lshkm_cube;
typedef struct lshkm_vectors_s* lshkm_vectors;
typedef struct lshkm_tweets_s* lshkm_tweets;

/* ------------------------------------------------------------------ context */
const char* lshkm_last_error(void);
const char* lshkm_version(void);
/* pow(x, 2) as the reference computes it (glibc's pow, cust_vector.hpp:132):
 * out_dev[i] for x_dev[i], i < n, on the device (csrc/gpow2.h). */
int lshkm_pow2(lshkm_ctx ctx, const double* x_dev, int64_t n, double* out_dev);
/* Host-only (no GPU): compares the device's restatement of glibc's pow(x, 2)
 * (the same code, compiled for the host) with this process's own pow on a
 * fixed set of inputs whose squares lie near rounding midpoints (the inputs
 * that tell pow from x*x) plus exact ties and special ranges; *mismatches_host
 * = how many differ (0 when the process's libm is the one the restatement
 * follows), *tested_host = inputs tried. */
int lshkm_pow_selfcheck(int64_t* mismatches_host, int64_t* tested_host);
/* A context on `device` (gfx950). Fails with LSHKM_ERR_UNSUPPORTED, before any
 * device work, when this process's pow(x, 2) differs from the restatement
 * (the pow contract above; checked once per process). */
int lshkm_ctx_create(int device, lshkm_ctx* out);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream), used
 * verbatim: NULL is the default (null) stream. A new context uses its own stream. */
int lshkm_ctx_set_stream(lshkm_ctx ctx, void* hip_stream);
/* Distance contract of the context (see Conventions): LSHKM_DIST_CERTIFIED
 * (the default of a new context) or LSHKM_DIST_EXACT (the reference's
 * euclideanDistance, cust_vector.hpp:124-136, for every row; a few percent
 * slower at d = 128). The context's mode alone decides (no environment
 * override in this library). */
int lshkm_ctx_set_dist_mode(lshkm_ctx ctx, int mode);
int lshkm_ctx_get_dist_mode(lshkm_ctx ctx, int* mode_host);
int lshkm_ctx_sync(lshkm_ctx ctx);
int lshkm_ctx_destroy(lshkm_ctx ctx);
/* Device memory for callers without HIP headers (the C++ shim
 * include/lshkm_compat.hpp, cgo/JNI bindings). Copies are ordered on the
 * context's stream and complete before return; free waits for the stream. */
int lshkm_dev_alloc(lshkm_ctx ctx, int64_t bytes, void** out_dev);
int lshkm_dev_free(lshkm_ctx ctx, void* p_dev);
int lshkm_memcpy_h2d(lshkm_ctx ctx, void* dst_dev, const void* src_host, int64_t bytes);
int lshkm_memcpy_d2h(lshkm_ctx ctx, void* dst_host, const void* src_dev, int64_t bytes);
/* Counters: 0 = hash values resolved by the exact soft-x87 path,
 * 1 = points whose argmin needed the exact all-centroid pass,
 * 2 = k-means++ prefix-sum chunks walked, 3 = of which summed element by element,
 * 4 = cosine Lloyd winner distances the certified fast form declined (soft-x87 chain),
 * 5 = rows the hi-only fused pass (one f16 product per score) left to the 3-product form,
 * 6 = rows the fused pass listed for the hash fix-up,
 * 7 = clustering-recommender similarities decided by the x87 chain (lshkm_cluster_top_n),
 * 8 = euclidean winner distances (LSHKM_DIST_EXACT, hi-only pass) whose chain met an
 *     inexact square and were redone with glibc's pow(x, 2) (gpow2.h),
 * 9 = k-means (cluster, dim) sums of fp32 rows whose never-rounds test failed,
 *     i.e. that took a rounding-aware chain instead of plain fp64 adds,
 * 10 = PAM update: clusters whose argmin went through the MFMA screen,
 * 11 = PAM update: members of those clusters the screen left to the exact chain,
 * 12 = lshkm_lsh_p_closest / lshkm_cube_p_closest: users the MFMA screen settled,
 * 13 = ... users sent to the lists path (a poison row or user, a kept-list
 *      overflow, a tie or a NaN among the first P + 1; every user of a call the
 *      screen does not take),
 * 14 = ... candidates the screen kept for the exact pass,
 * 15 = ... candidates the screen saw,
 * 16 = of counter 1's points, those the fused pass's refinement named the only
 *      two possible nearest centroids of (decided between the two alone),
 * 17 = lshkm_min_vector_dist: queries the MFMA screen settled,
 * 18 = ... queries sent to the exact scan over all rows (a poison query, a
 *      kept-list overflow; every query of a call the screen does not take),
 * 19 = ... exact distances the settle computed (kept and poison rows; the lists
 *      form's list entries),
 * 20 = lshkm_knn: queries the MFMA screen settled,
 * 21 = ... queries sent to the exact scan over all rows (a poison query, fewer
 *      than k row groups with a real row, a kept-list overflow; every query of
 *      a call the screen does not take),
 * 22 = ... exact distances the settle computed (kept and poison rows; the lists
 *      form's list entries). */
int lshkm_get_stat(lshkm_ctx ctx, int which, int64_t* value_host);
int lshkm_reset_stats(lshkm_ctx ctx);
/* HIP-event timing of the dominant kernel launch (the fused hash+assign kernel)
 * on the context's stream; lshkm_last_kernel_ms waits for and returns the last one. */
int lshkm_ctx_enable_timing(lshkm_ctx ctx, int on);
int lshkm_last_kernel_ms(lshkm_ctx ctx, float* ms_host);

/* ------------------------------------------- parameter generation (host)
 * std::default_random_engine seeded with `seed`, draws in the reference's
 * order; *rng_state_host receives the engine state after the last draw.
 * Replaces the generator constructors:
 *   EuclideanPhiGen  lib/generators/euclidean_phi_gen.hpp:59-71 (via euclidean_h_gen.hpp:56-69)
 *   CosineGGen       lib/generators/cosine_g_gen.hpp:48-52     (via cosine_h_gen.hpp:53-60)
 *   create_hypercube lib/lsh_cube.hpp:112-126                  (EuclideanFGen / CosineHGen) */
int lshkm_params_lsh_euclidean(uint64_t seed, int L, int k, int d, float w,
                               float* V_host /*[L][k][d]*/, float* t_host /*[L][k]*/,
                               int32_t* r_host /*[L][k]*/, uint32_t* rng_state_host);
int lshkm_params_lsh_cosine(uint64_t seed, int L, int k, int d, double* R_host /*[L][k][d]*/,
                            uint32_t* rng_state_host);
int lshkm_params_cube_euclidean(uint64_t seed, int k, int d, float w, float* V_host /*[k][d]*/,
                                float* t_host /*[k]*/, uint32_t* rng_state_host);
int lshkm_params_cube_cosine(uint64_t seed, int k, int d, double* R_host /*[k][d]*/,
                             uint32_t* rng_state_host);

/* ---------------------------------------------------------------- LSH index
 * create_LSH_hashtables (lsh_cube.hpp:44-74): metric EUCLIDEAN uses
 * EuclideanPhiGen with nb = N / lsh_bucket_div buckets; COSINE uses CosineGGen
 * with 2^k buckets (nb ignored). Parameters are copied to the device.
 * V/t/r for EUCLIDEAN, R for COSINE (the other may be NULL). */
int lshkm_lsh_create(lshkm_ctx ctx, int metric, int d, int k, int L, int64_t nb, float w,
                     const float* V_host, const float* t_host, const int32_t* r_host,
                     const double* R_host, lshkm_lsh* out);
int lshkm_lsh_destroy(lshkm_lsh lsh);
/* Hash a batch without inserting: EuclideanPhiGen::generate
 * (euclidean_phi_gen.hpp:77-92) + mod(phi, nb) (cust_hashtable.hpp:68).
 * tuples_dev [N][L][k] (EUCLIDEAN only), phi_dev [N][L], bucket_dev [N][L];
 * any output may be NULL. For COSINE phi == bucket == g. */
int lshkm_lsh_hash(lshkm_lsh lsh, const float* X_dev, int64_t N, int32_t* tuples_dev,
                   int32_t* phi_dev, int32_t* bucket_dev);
int lshkm_lsh_hash_f64(lshkm_lsh lsh, const double* X_dev, int64_t N, int32_t* tuples_dev,
                       int32_t* phi_dev, int32_t* bucket_dev);
/* Insert all N rows (create_LSH_hashtables' insert loop, lsh_cube.hpp:69-70):
 * hashes, then a stable bucket scatter (member order = row order,
 * vector_bucket.hpp:41-44). The dataset rows and their tuples stay
 * device-resident in the handle (X_dev must stay valid for queries that use
 * alias rows only through their tuples; it is not read again). */
int lshkm_lsh_build(lshkm_lsh lsh, const float* X_dev, int64_t N);
int lshkm_lsh_build_f64(lshkm_lsh lsh, const double* X_dev, int64_t N);
/* Bucket contents of one table (getBucketFromIndex, cust_hashtable.hpp:116-119):
 * row_ptr_host [nb+1], idx_host [N]. */
int lshkm_lsh_get_buckets(lshkm_lsh lsh, int table, int64_t* row_ptr_host, int32_t* idx_host);
/* Device views of the built index (valid until destroy/rebuild). */
int lshkm_lsh_device_views(lshkm_lsh lsh, const int64_t** row_ptr_dev /*[L][nb+1]*/,
                           const int32_t** idx_dev /*[L][N]*/, const int32_t** tuples_dev /*[N][L][k]*/,
                           const int32_t** bucket_dev /*[N][L]*/);
/* Batched queries (get_LSH_filtered_combined_buckets, lsh_cube.hpp:93-106,
 * or get_LSH_combined_buckets :77-90 when filtered == 0). Output per query:
 * the deduplicated union of its L buckets, ascending row index (std::set
 * order). alias_rows_dev[q] >= 0 says "query q has the ID of dataset row r":
 * the reference's first-write-wins ID map (euclidean_phi_gen.hpp:94) then
 * filters with row r's tuple. May be NULL.
 * Two-phase: out_ptr_dev [nq+1] always written (prefix offsets); rows are
 * written to out_idx_dev only if total <= out_cap. *total_host = total rows.
 * A filling call (out_idx_dev != NULL) right after a sizing call (NULL) with
 * the same Q_dev, nq, alias_rows_dev, filtered and out_ptr_dev buffer -- and no
 * other call on the context's workspace in between -- reuses the sizing call's
 * device state: the contents of Q, alias and out_ptr must not change between
 * the two calls. Any other filling call recomputes everything. */
int lshkm_lsh_query(lshkm_lsh lsh, const float* Q_dev, int64_t nq, const int32_t* alias_rows_dev,
                    int filtered, int64_t* out_ptr_dev, int32_t* out_idx_dev, int64_t out_cap,
                    int64_t* total_host);
int lshkm_lsh_query_f64(lshkm_lsh lsh, const double* Q_dev, int64_t nq, const int32_t* alias_rows_dev,
                        int filtered, int64_t* out_ptr_dev, int32_t* out_idx_dev, int64_t out_cap,
                        int64_t* total_host);

/* ---------------------------------------------------------------- hypercube
 * create_hypercube (lsh_cube.hpp:108-136): k EuclideanFGen (V,t,w + the lazy
 * coin engine state rng_state) or k CosineHGen (R); 2^k buckets. */
int lshkm_cube_create(lshkm_ctx ctx, int metric, int d, int k, float w, const float* V_host,
                      const float* t_host, const double* R_host, uint32_t rng_state, lshkm_cube* out);
int lshkm_cube_destroy(lshkm_cube cube);
/* Insert N rows: vertices (HypercubeGen::generate, hypercube_gen.hpp:63-73)
 * with EuclideanF coins drawn on first sight of each h in (row, f) order
 * (euclidean_f_gen.hpp:65-79), then the stable scatter into 2^k buckets. */
int lshkm_cube_build(lshkm_cube cube, const float* X_dev, int64_t N);
int lshkm_cube_build_f64(lshkm_cube cube, const double* X_dev, int64_t N);
/* Vertices of a query batch (getHash, cust_hashtable.hpp:122-125). Unseen h
 * values draw new coins in (query, f) order from the continued engine. */
int lshkm_cube_vertices(lshkm_cube cube, const float* Q_dev, int64_t nq, int32_t* vertex_dev);
int lshkm_cube_vertices_f64(lshkm_cube cube, const double* Q_dev, int64_t nq, int32_t* vertex_dev);
int lshkm_cube_get_buckets(lshkm_cube cube, int64_t* row_ptr_host /*[2^k+1]*/, int32_t* idx_host /*[N]*/);
/* get_hypercube_combined_buckets (lsh_cube.hpp:139-177): main bucket then
 * `probes` neighbours in get_num_hamming_dist_from order (utils.cpp:22-50),
 * probes == 1 skipping distance 1 as the reference does. Two-phase like
 * lshkm_lsh_query. */
int lshkm_cube_query(lshkm_cube cube, const float* Q_dev, int64_t nq, int probes,
                     int64_t* out_ptr_dev, int32_t* out_idx_dev, int64_t out_cap, int64_t* total_host);
int lshkm_cube_query_f64(lshkm_cube cube, const double* Q_dev, int64_t nq, int probes,
                         int64_t* out_ptr_dev, int32_t* out_idx_dev, int64_t out_cap, int64_t* total_host);
/* Sharded build of the euclidean cube (the coins of
 * euclidean_f_gen.hpp:65-79 must be drawn in GLOBAL first-occurrence order):
 * 1. each shard: lshkm_cube_unseen -> the (f, h) pairs of its rows that have
 *    no coin yet, with their first local row (row_host; add the shard's row0);
 *    if *count_host > cap nothing is copied and the call may be repeated;
 * 2. all-gather, keep each (f, h) at its smallest global (row * k + f), sort by
 *    it, and draw with lshkm_coins_draw (identical on every rank);
 * 3. each shard: lshkm_cube_import_coins (memo + the engine state after the
 *    draws), then lshkm_cube_build (no coin left to draw). */
int lshkm_cube_unseen(lshkm_cube cube, const float* X_dev, int64_t N, int32_t* f_host, int32_t* h_host,
                      int64_t* row_host, int64_t cap, int64_t* count_host);
int lshkm_cube_unseen_f64(lshkm_cube cube, const double* X_dev, int64_t N, int32_t* f_host, int32_t* h_host,
                          int64_t* row_host, int64_t cap, int64_t* count_host);
int lshkm_cube_import_coins(lshkm_cube cube, const int32_t* f_host, const int32_t* h_host, const int32_t* bit_host,
                            int64_t n, uint32_t rng_state);
/* Host draw of n coins in order from *rng_state (minstd_rand0 state, updated):
 * bit[i] = mod(h[i], uniform_int_distribution<int>(1, 2)). No device needed. */
int lshkm_coins_draw(uint32_t* rng_state, const int32_t* h_host, int64_t n, int32_t* bit_host);
/* Coin memo export: f_host/h_host/bit_host [cap]; *count_host = entries. */
int lshkm_cube_get_memo(lshkm_cube cube, int32_t* f_host, int32_t* h_host, int32_t* bit_host,
                        int64_t cap, int64_t* count_host, uint32_t* rng_state_host);

/* ------------------------------------------------------------------ k-means
 * lloyds_assignment (assignment.hpp:54-80): for each row the centroid with the
 * smallest distance (strict '<', first index wins), its fp64 distance, then
 * the centroid override: assign[src_rows[c]] = c, dist = 0 for c = 0..K-1
 * (src_rows_host may be NULL; entries outside [0, N) are ignored). */
int lshkm_lloyd_assign(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const double* C_dev,
                       int K, int metric, const int32_t* src_rows_host, int32_t* assign_dev,
                       double* dist_dev);
int lshkm_lloyd_assign_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const double* C_dev,
                           int K, int metric, const int32_t* src_rows_host, int32_t* assign_dev,
                           double* dist_dev);
/* The hot path in one pass over the points: LSH hashing of the rows
 * (EuclideanPhiGen::generate for every table, euclidean_phi_gen.hpp:77-92, and
 * the bucket index of cust_hashtable.hpp:68) and lloyds_assignment
 * (assignment.hpp:54-80) against C_dev. Outputs as lshkm_lsh_hash and
 * lshkm_lloyd_assign (tuples/phi/bucket may be NULL). Same results as the two
 * calls; one read of X when the index is euclidean with d = 128, L*k <= 32. */
int lshkm_hash_assign(lshkm_lsh lsh, const float* X_dev, int64_t N, const double* C_dev, int K,
                      const int32_t* src_rows_host, int32_t* tuples_dev, int32_t* phi_dev, int32_t* bucket_dev,
                      int32_t* assign_dev, double* dist_dev);
int lshkm_hash_assign_f64(lshkm_lsh lsh, const double* X_dev, int64_t N, const double* C_dev, int K,
                          const int32_t* src_rows_host, int32_t* tuples_dev, int32_t* phi_dev, int32_t* bucket_dev,
                          int32_t* assign_dev, double* dist_dev);
/* The same with the assignment metric chosen (lshkm_hash_assign is euclidean
 * Lloyd): main.cpp's cosine flow (main.cpp:150-160, 196) hashes with the
 * cosine family and clusters with cosineDistance. One read of X when the index
 * metric equals the assignment metric, d = 128, L*k <= 32 (cosine: k = 4). */
int lshkm_hash_assign_metric(lshkm_lsh lsh, const float* X_dev, int64_t N, const double* C_dev, int K, int metric,
                             const int32_t* src_rows_host, int32_t* tuples_dev, int32_t* phi_dev, int32_t* bucket_dev,
                             int32_t* assign_dev, double* dist_dev);
int lshkm_hash_assign_metric_f64(lshkm_lsh lsh, const double* X_dev, int64_t N, const double* C_dev, int K,
                                 int metric, const int32_t* src_rows_host, int32_t* tuples_dev, int32_t* phi_dev,
                                 int32_t* bucket_dev, int32_t* assign_dev, double* dist_dev);
/* k_means (update.hpp:37-86): exact-order per-cluster fp64 sums in row order,
 * divided by the count unless empty; *cont_host = 1 iff some center moved
 * more than min_dist. C_new_dev [K][d], counts_dev [K] (may be NULL). N = 0
 * (X_dev and assign_dev may then be NULL; also lshkm_kmeans_partial): every
 * cluster is empty, every sum +0.0. */
int lshkm_kmeans_update(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int32_t* assign_dev,
                        const double* C_old_dev, int K, int metric, double min_dist,
                        double* C_new_dev, int64_t* counts_dev, int* cont_host);
int lshkm_kmeans_update_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int32_t* assign_dev,
                            const double* C_old_dev, int K, int metric, double min_dist,
                            double* C_new_dev, int64_t* counts_dev, int* cont_host);
/* Sharded update (fast mode): per-shard exact-order sums, no division.
 * sums_dev [K][d], counts_dev [K]. Combine across ranks with an all-reduce,
 * then lshkm_kmeans_finalize. */
int lshkm_kmeans_partial(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int32_t* assign_dev,
                         int K, double* sums_dev, int64_t* counts_dev);
int lshkm_kmeans_partial_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int32_t* assign_dev,
                             int K, double* sums_dev, int64_t* counts_dev);
/* lshkm_kmeans_partial over the cluster CSR lshkm_clusters returned for the
 * same assignment (crow_dev [K+1], rows_dev [N]): the same sums without a
 * second sort when the caller needs the CSR anyway (the C5 iteration's
 * recommend step, main.cpp:261 over separate_clusters_from_input). */
int lshkm_kmeans_partial_csr(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int64_t* crow_dev,
                             const int32_t* rows_dev, int K, double* sums_dev, int64_t* counts_dev);
int lshkm_kmeans_partial_csr_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int64_t* crow_dev,
                                 const int32_t* rows_dev, int K, double* sums_dev, int64_t* counts_dev);
/* Sharded update (exact mode): the per-(c, j) chains continue from
 * carry_sums_dev / carry_counts_dev (the previous shard's result, or NULL for
 * the first shard), so passing the carry shard to shard in row order gives the
 * reference's single sequential sum (update.hpp:45-58) bit for bit.
 * carry_sums_dev must be a previous call's sums_dev, or NULL (a chain started
 * at +0.0 never yields -0.0, and no form is specified for a -0.0 carry). */
int lshkm_kmeans_partial_carry(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int32_t* assign_dev,
                               int K, const double* carry_sums_dev, const int64_t* carry_counts_dev,
                               double* sums_dev, int64_t* counts_dev);
int lshkm_kmeans_partial_carry_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d,
                                   const int32_t* assign_dev, int K, const double* carry_sums_dev,
                                   const int64_t* carry_counts_dev, double* sums_dev, int64_t* counts_dev);
/* Sharded update, bit-exact at all-reduce cost (the reference's
 * one sequential chain per (c, j), update.hpp:45-58, over row shards in rank
 * order). crow_dev / rows_dev: this rank's cluster CSR (lshkm_clusters).
 *  1. lshkm_kmeans_shard_begin: this rank's per-(c, j) partial sums (any
 *     order) sums_dev [K][d], the sums of |x| asum_dev [K][d], qt_dev [2][K][d]
 *     int32 (the lowest set-bit exponent of the values, then minus the top
 *     bit position), counts_dev [K].
 *  2. exchange: all-gather sums_dev in rank order into gathered [world][K][d];
 *     all-reduce asum_dev and counts_dev (SUM) and qt_dev (MIN).
 *  3. lshkm_kmeans_shard_certify (identical on every rank): per (c, j) the
 *     never-rounds test on the global values. Where it holds, every partial sum
 *     of any subset of the chain's values in any order is a double, so the
 *     total of the gathered partials IS the reference's chain: sums_out_dev.
 *     Elsewhere mask_dev [K][d] != 0: 2 for a chain of at most 32,768 values
 *     in all (one lane each in the chain phase), else 1 and flag_dev [K] has
 *     bit min(31, j / 64) set (segment records); start_dev [K][d] (may be
 *     NULL) = the chain's approximate value
 *     before this rank's rows (the lower ranks' partials); *n_flagged_host =
 *     the number of (c, j) masked (the same on every rank).
 *  4. only when *n_flagged_host > 0: lshkm_kmeans_shard_prepare (the lane
 *     list and the masked chains' binade-segment records from start_dev; all
 *     ranks at once), then
 *     in rank order lshkm_kmeans_shard_chain: the masked chains continued over
 *     this rank's rows from the previous rank's sums_out (carry_dev; NULL on
 *     rank 0), written into sums_dev where mask_dev is set; send sums_dev on.
 *     The last rank's sums_dev holds every chain's result: broadcast it.
 * ws_dev (prepare / chain; the same buffer for both): at least
 * lshkm_kmeans_shard_ws_bytes bytes, holding the records between the calls.
 * Then lshkm_kmeans_finalize on the totals and the all-reduced counts. One
 * rank (world 1) is the single-GPU update. sharding.kmeans_sums_sharded runs
 * the protocol over torch.distributed (RCCL on GPUs). */
int lshkm_kmeans_shard_begin(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int64_t* crow_dev,
                             const int32_t* rows_dev, int K, double* sums_dev, double* asum_dev, int32_t* qt_dev,
                             int64_t* counts_dev);
int lshkm_kmeans_shard_begin_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int64_t* crow_dev,
                                 const int32_t* rows_dev, int K, double* sums_dev, double* asum_dev, int32_t* qt_dev,
                                 int64_t* counts_dev);
int lshkm_kmeans_shard_certify(lshkm_ctx ctx, int K, int d, int world, int rank, const double* gathered_dev,
                               const double* asum_dev, const int32_t* qt_dev, const int64_t* counts_dev,
                               double* sums_out_dev, double* start_dev, int32_t* flag_dev, uint8_t* mask_dev,
                               int64_t* n_flagged_host);
int lshkm_kmeans_shard_ws_bytes(int64_t N, int K, int d, int64_t* bytes_host);
int lshkm_kmeans_shard_prepare(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int64_t* crow_dev,
                               const int32_t* rows_dev, int K, const double* start_dev, const int32_t* flag_dev,
                               const uint8_t* mask_dev, void* ws_dev, int64_t ws_bytes);
int lshkm_kmeans_shard_prepare_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int64_t* crow_dev,
                                   const int32_t* rows_dev, int K, const double* start_dev, const int32_t* flag_dev,
                                   const uint8_t* mask_dev, void* ws_dev, int64_t ws_bytes);
int lshkm_kmeans_shard_chain(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int64_t* crow_dev,
                             const int32_t* rows_dev, int K, const int32_t* flag_dev, const uint8_t* mask_dev,
                             const double* carry_dev, void* ws_dev, int64_t ws_bytes, double* sums_dev);
int lshkm_kmeans_shard_chain_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int64_t* crow_dev,
                                 const int32_t* rows_dev, int K, const int32_t* flag_dev, const uint8_t* mask_dev,
                                 const double* carry_dev, void* ws_dev, int64_t ws_bytes, double* sums_dev);
int lshkm_kmeans_finalize(lshkm_ctx ctx, const double* sums_dev, const int64_t* counts_dev, int K, int d,
                          const double* C_old_dev, int metric, double min_dist, double* C_new_dev,
                          int* cont_host);
/* separate_clusters_from_input (utils.hpp:150-158): the clusters' member lists
 * as a CSR, cluster c = rows_dev[crow_dev[c] .. crow_dev[c+1]) in row order
 * (the insertion order of the reference's per-cluster vectors). assign_dev
 * values must lie in [0, K) (what lshkm_lloyd_assign writes). crow_dev [K+1],
 * rows_dev [N]. */
int lshkm_clusters(lshkm_ctx ctx, const int32_t* assign_dev, int64_t N, int K, int64_t* crow_dev,
                   int32_t* rows_dev);

/* ------------------------------------------------------------- PAM update
 * pam_lloyds (update.hpp:89-142): per cluster (members in row order) the
 * member p with the smallest dist_sum(p) = sum_j dist(x_p, x_j) over all
 * members j in member order (j = p included), sequential fp64 adds from 0.0,
 * every distance the reference's exact one; selection by
 * `if (min == -1 || s < min)` in member order (the first of equal sums; the
 * first member whatever its sum; a NaN min is never replaced). The reference's
 * "<id>to<id>" cache needs no model: d is bitwise symmetric for unique IDs.
 * prev_rows_host[c]: the row the previous centroid of c is (-1: not a data
 * row, e.g. a "k_means_center"; NULL: all -1). medoid_rows_host [K]: the chosen
 * rows (may be the prev_rows_host buffer); C_new_dev [K][d] (with C_old_dev; both
 * NULL or neither): those rows widened to fp64; sums_host [K] (may be NULL):
 * the winning dist_sum, NaN bits as x86 produces them; *swapped_host = 1 iff
 * some cluster's medoid_rows[c] != prev_rows[c] (-1 always counts), the
 * reference's return value.
 * The one departure: an empty cluster (the reference indexes an empty vector,
 * undefined) keeps its previous centroid: medoid_rows[c] = prev_rows[c],
 * C_new[c] = C_old[c], sums[c] = -1.0 (the untouched sentinel), not a swap.
 * assign values outside [0, K) are LSHKM_ERR_ARG. N < 2^31. Workspace is
 * O(N + K): no cluster's distance matrix is stored. Euclidean clusters of
 * enough members (d <= 128, finite rows with |x| < 2^50) first pass a screen
 * on the matrix cores that bounds every member's dist_sum rigorously; only the
 * members that can still hold the minimum take the exact chain, so the result
 * is the same bit for bit (counters 10, 11). */
int lshkm_pam_update(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int32_t* assign_dev, int K,
                     int metric, const int32_t* prev_rows_host, const double* C_old_dev,
                     int32_t* medoid_rows_host, double* C_new_dev, double* sums_host, int* swapped_host);
int lshkm_pam_update_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int32_t* assign_dev, int K,
                         int metric, const int32_t* prev_rows_host, const double* C_old_dev,
                         int32_t* medoid_rows_host, double* C_new_dev, double* sums_host, int* swapped_host);

/* --------------------------------------------------------- range assignment
 * lsh_range_assignment / cube_range_assignment (assignment.hpp:108-145):
 * remove_clustering, range_assignment (:148-217) over the combined buckets of
 * the centroids, lloyds_for_remaining (:83-104) for the rows left unassigned,
 * then the centroid override (src_rows_host as in lshkm_lloyd_assign).
 * comb_ptr_dev [K+1] / comb_idx_dev: centroid i's combined bucket, in the
 * reference's order — what lshkm_lsh_query (filtered = 0) or lshkm_cube_query
 * returns for the centroid rows. Radius: find_min_vector_distance of the
 * centroids / 2 (utils.hpp:161-178), doubled after every centroid.
 * key_host [K] (may be NULL = all distinct): the reference caches distances by
 * "<centroid id>to<row id>" (:176-186), so centroids with the same ID share
 * entries (every "k_means_center" after k_means): give them equal keys.
 * *passes_host (may be NULL) = passes of the do-while loop. N < 2^31. */
int lshkm_range_assign(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const double* C_dev, int K, int metric,
                       const int64_t* comb_ptr_dev, const int32_t* comb_idx_dev, const int32_t* key_host,
                       const int32_t* src_rows_host, int32_t* assign_dev, double* dist_dev, int* passes_host);
int lshkm_range_assign_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const double* C_dev, int K,
                           int metric, const int64_t* comb_ptr_dev, const int32_t* comb_idx_dev,
                           const int32_t* key_host, const int32_t* src_rows_host, int32_t* assign_dev,
                           double* dist_dev, int* passes_host);

/* --------------------------------------------------------------- silhouette
 * silhouette_cluster (silhouette.hpp:31-80) over the clusters of `assign`
 * (separate_clusters_from_input, utils.hpp:150-158: members in row order)
 * with the K centroids C_dev (nearest other centroid = neighbour cluster).
 * out_host [K+1]: per-cluster mean s(i), then the overall mean; s_dev [N]
 * (may be NULL): silhouette_of_i of every row (:83-144). Exact distances in
 * the reference's order; NaNs as x86 produces them (empty cluster: 0/0). */
int lshkm_silhouette(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int32_t* assign_dev,
                     const double* C_dev, int K, int metric, double* out_host, double* s_dev);
int lshkm_silhouette_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int32_t* assign_dev,
                         const double* C_dev, int K, int metric, double* out_host, double* s_dev);

/* ----------------------------------------------------------- initialization
 * k_means_pp (initialization.hpp:71-156): the K dataset rows chosen as initial
 * centroids (centroids[i] = &input_vectors[rows_host[i]]), with
 * std::default_random_engine seeded with `seed` (the reference reads the
 * clock). D^2 seeding with the reference's exact distances, (min/max)^2
 * prefix sums in row order and its binary search. Assumes unique vector IDs
 * (the reference's distance cache is keyed by them). N < 2^31, d <= 4096. */
int lshkm_kmeans_pp(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, int K, int metric, uint64_t seed,
                    int32_t* rows_host);
int lshkm_kmeans_pp_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, int K, int metric, uint64_t seed,
                        int32_t* rows_host);
/* k_means_pp over contiguous row shards in rank order (rank r holds rows
 * [row0_r, row0_r + n_r) of N_total; n_r = 0 is legal in every call and
 * touches no memory), bit for bit lshkm_kmeans_pp on the concatenated rows.
 * lshkm_kpp_draws (host only, identical on every rank): the engine's draws in
 * the reference's order -- *first_row_host (:75-79), then one canonical
 * uniform_real<double>(0, 1) per new centroid, canon_host[1..K-1] (:132-133;
 * canon_host[0] = 0): uniform_real(0, total) is canon * (total - 0) + 0.
 * A later row needs from the earlier ones only the max of the minima
 * (:117-118) and the running prefix sum (:123-129), so per new centroid
 * i = 1..K-1 every rank runs, with the host and the exchange between the calls
 * (sharding.kmeans_pp_sharded runs it over torch.distributed):
 *  1. lshkm_kpp_shard_dist: the rows' distances to centroid i - 1 (c_dev: its
 *     [d] row, of the rows' type; :93-119) folded into the running minima kept
 *     in ws_dev; *max_bits_host = the shard's max of minima as a bit pattern
 *     (0 if none is > 0), *sum_host = its approximate sum of min^2. it = i.
 *  2. exchange: all-gather the pairs. The global max is the largest bit
 *     pattern; start = (the lower ranks' sums) / max^2 approximates the prefix
 *     sum before this shard.
 *  3. lshkm_kpp_shard_units: (min / max)^2 of every row with the GLOBAL max
 *     (:123-127) and the chunk guesses from `start` (a guess: a wrong one
 *     costs time, never correctness).
 *  4. in rank order lshkm_kpp_shard_chain: the sequential fp64 chain (:128)
 *     continued from s_in (the previous rank's *s_out_host; 0 on the first)
 *     over this rank's rows; send *s_out_host on. The last rank's is the total
 *     (:132): broadcast it.
 *  5. rd = canon[i] * (total - 0) + 0 in fp64 (:132-133, canon from
 *     lshkm_kpp_draws), then lshkm_kpp_shard_pick: *row_host = the first local
 *     row whose prefix sum is >= rd, or -1; with owns_row0 (the rank holding
 *     global row 0) row 0 unless rd > its prefix sum (:139, a NaN rd
 *     included). The chosen row (:134-149) is the minimum of row0 + *row_host
 *     over the ranks that found one.
 * ws_dev: at least lshkm_kpp_shard_ws_bytes(n) bytes, the same buffer through
 * all K - 1 iterations (it holds the minima). The chain adds to the counters
 * the single-device walk uses. n < 2^31, d <= 4096. */
int lshkm_kpp_draws(uint64_t seed, int64_t N_total, int K, int64_t* first_row_host, double* canon_host);
int lshkm_kpp_shard_ws_bytes(int64_t n, int64_t* bytes_host);
int lshkm_kpp_shard_dist(lshkm_ctx ctx, const float* X_dev, int64_t n, int d, int metric, const float* c_dev, int it,
                         void* ws_dev, int64_t ws_bytes, uint64_t* max_bits_host, double* sum_host);
int lshkm_kpp_shard_dist_f64(lshkm_ctx ctx, const double* X_dev, int64_t n, int d, int metric, const double* c_dev,
                             int it, void* ws_dev, int64_t ws_bytes, uint64_t* max_bits_host, double* sum_host);
int lshkm_kpp_shard_units(lshkm_ctx ctx, int64_t n, uint64_t gmax_bits, double start, void* ws_dev,
                          int64_t ws_bytes);
int lshkm_kpp_shard_chain(lshkm_ctx ctx, int64_t n, double s_in, void* ws_dev, int64_t ws_bytes,
                          double* s_out_host);
int lshkm_kpp_shard_pick(lshkm_ctx ctx, int64_t n, double rd, int owns_row0, void* ws_dev, int64_t ws_bytes,
                         int64_t* row_host);
/* rand_selection (initialization.hpp:39-69): K distinct rows drawn uniformly,
 * redrawing on a repeat. Host only. 1 <= K <= N. */
int lshkm_rand_selection(uint64_t seed, int64_t N, int K, int32_t* rows_host);

/* ----------------------------------------------------------- recommendation
 * get_P_closest (crypto_rec.hpp:213-231) for nq users at once. User q's
 * neighbours are the dataset rows cand_idx_dev[cand_ptr_dev[q] ..
 * cand_ptr_dev[q+1]) in the order the reference's neighbour vector holds them
 * (ascending row: a query's output). Similarity = cosineSimilarity(neighbour,
 * user) (cust_vector.hpp:158-174); order = the reference's quicksort
 * (parallel_quickSort, :234-277, ties and NaNs included); first P kept.
 * Rows are fp64 (X_dev [N][d] neighbour pool, U_dev [nq][d] users).
 * out_idx_dev / out_sim_dev [nq][P] (-1 / 0 past the count), out_cnt_dev [nq]
 * = min(P, neighbours). Bit-exact on any doubles (the norms' squares are
 * glibc's pow(x, 2)). */
int lshkm_p_closest(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const double* U_dev, int64_t nq,
                    const int64_t* cand_ptr_dev, const int32_t* cand_idx_dev, int P, int32_t* out_idx_dev,
                    double* out_sim_dev, int32_t* out_cnt_dev);
/* main.cpp:160-162 for nq users at once: get_LSH_filtered_combined_buckets
 * (lsh_cube.hpp:93-106) followed by get_P_closest (crypto_rec.hpp:213-231),
 * without the neighbour vectors. out_idx_dev / out_sim_dev / out_cnt_dev are bit
 * for bit what lshkm_lsh_query_f64(filtered = 1, alias NULL) ->
 * lshkm_cv_exclude(excl_lo, excl_hi) -> lshkm_p_closest produce, on any doubles
 * (ties, NaNs, zero rows, empty neighbourhoods). X_dev [N][d]: the fp64 rows lsh
 * was built over; U_dev [nq][d]; rows in [excl_lo, excl_hi) are no one's
 * neighbours (merge_except_for; excl_lo == excl_hi: none). ncand_dev [nq] or
 * NULL: each user's neighbour count. A cosine handle with d <= 128, L * k <= 32
 * and P <= 447 goes through an f32 MFMA screen with a rigorous bound (DESIGN.md
 * 5c) that leaves only the candidates near a user's P best to the exact chain and
 * never writes a candidate list; everything else, and every user the screen
 * cannot decide, runs the sequence above in chunks of bounded size. The handle
 * must be built (LSHKM_ERR_STATE); P < 1 or excl_lo > excl_hi is LSHKM_ERR_ARG.
 * nq < 2^31. Returns after its workspace is free for the next call. */
int lshkm_lsh_p_closest(lshkm_lsh lsh, const double* X_dev, const double* U_dev, int64_t nq, int32_t excl_lo,
                        int32_t excl_hi, int P, int32_t* out_idx_dev, double* out_sim_dev, int32_t* out_cnt_dev,
                        int64_t* ncand_dev);
/* The same from a built hypercube: get_hypercube_combined_buckets
 * (lsh_cube.hpp:138-177) followed by get_P_closest, without the neighbour
 * vectors. out_idx_dev / out_sim_dev / out_cnt_dev are bit for bit what
 * lshkm_cube_query_f64(cube, U, nq, probes) -> lshkm_p_closest produce, on any
 * doubles (ties, NaNs, zero rows, empty neighbourhoods); ncand_dev [nq] or NULL:
 * each user's combined bucket's length. X_dev [N][d]: the fp64 rows the cube was
 * built over (lshkm_cube_build_f64); U_dev [nq][d]; probes as lshkm_cube_query
 * takes it. The handle is left as lshkm_cube_query_f64 on the same users leaves
 * it (the euclidean cube's coin memo and engine state). Either metric with
 * d <= 128 and P <= 447 goes through the f32 MFMA screen of lshkm_lsh_p_closest
 * (a row is a user's candidate iff the XOR of their vertices is a probe mask;
 * DESIGN.md 5e); everything else, and every user the screen cannot decide, runs
 * the sequence above in chunks of bounded size. The cube must be built
 * (LSHKM_ERR_STATE); P < 1 is LSHKM_ERR_ARG. nq < 2^31; nq == 0 writes nothing.
 * Returns after its workspace is free for the next call. */
int lshkm_cube_p_closest(lshkm_cube cube, const double* X_dev, const double* U_dev, int64_t nq, int probes, int P,
                         int32_t* out_idx_dev, double* out_sim_dev, int32_t* out_cnt_dev, int64_t* ncand_dev);
/* min_vector_euclidean_dist / min_vector_cosine_dist (lib/utils.hpp:107-140)
 * for nq queries at once: the exact nearest row of every query. dist_dev[q] is
 * bit for bit what the reference's helper returns for query Q[q] over the vector
 * of rows X: query.euclideanDistance(row) / query.cosineDistance(row)
 * (cust_vector.hpp:124-155: glibc's pow(x, 2) per square, the x87 inner product,
 * 1 - double(ip / denom)), the minimum taken by the reference's loop: start from
 * row 0, replace only on strict <. row_dev[q] (or NULL) is the row that holds it
 * (ours: the reference returns the value alone): of equal minima the lowest row.
 * If row 0's distance is a NaN the result is that NaN (x86's bits) and row 0,
 * since nothing is < NaN; a NaN at a later row is never taken. inf - inf, zero
 * rows under cosine and 1e+-200 entries are reproduced, not refused. N == 0:
 * dist = 0.0, row = -1 (utils.hpp:109-110); nq == 0 does no device work.
 * X_dev [N][d] and Q_dev [nq][d] share the element type (fp32, or fp64 with
 * _f64). The distances are the exact chain in both distance modes of the
 * context: one value per query leaves LSHKM_DIST_CERTIFIED nothing to save.
 * d <= 128 goes through an f32 MFMA screen over (query tile x row segment)
 * blocks with a rigorous bound that leaves only the rows that can
 * still hold the minimum to the exact chain; d > 128, and every query the screen
 * cannot decide (a poison query, more kept rows than the capacity), takes the
 * exact scan over all rows. N < 2^31, nq < 2^31, d >= 1, metric euclidean or
 * cosine, dist_dev not NULL: else LSHKM_ERR_ARG, before any device work.
 * Returns after its workspace is free for the next call. */
int lshkm_min_vector_dist(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const float* Q_dev, int64_t nq,
                          int metric, double* dist_dev /*[nq]*/, int32_t* row_dev /*[nq] or NULL*/);
int lshkm_min_vector_dist_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const double* Q_dev, int64_t nq,
                              int metric, double* dist_dev, int32_t* row_dev);
/* The same function over each query's own candidate vector
 * X[cand_idx_dev[cand_ptr_dev[q] .. cand_ptr_dev[q+1])], in list order: the
 * reference's helper applied to a combined bucket (the LSH / hypercube nearest
 * neighbour; lshkm_lsh_query's and lshkm_cube_query's CSR). Of equal minima the
 * first in the list wins; the NaN rule applies to the list's first element; an
 * empty list gives 0.0 and -1. row_dev[q] is the dataset row (cand_idx's value).
 * A cand_ptr that does not start at 0 or decreases, or an index outside [0, N),
 * is LSHKM_ERR_ARG (checked on the device before anything is written). */
int lshkm_min_vector_dist_lists(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const float* Q_dev, int64_t nq,
                                int metric, const int64_t* cand_ptr_dev /*[nq+1]*/, const int32_t* cand_idx_dev,
                                double* dist_dev, int32_t* row_dev);
int lshkm_min_vector_dist_lists_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const double* Q_dev,
                                    int64_t nq, int metric, const int64_t* cand_ptr_dev, const int32_t* cand_idx_dev,
                                    double* dist_dev, int32_t* row_dev);
/* The k exact nearest rows of every query: lshkm_min_vector_dist's distances,
 * the k smallest of them. The distance of (query, row) is bit for bit
 * query.euclideanDistance(row) / query.cosineDistance(row) (cust_vector.hpp:
 * 124-155: glibc's pow(x, 2) per square, the x87 inner product, 1 - double(ip /
 * denom)), the exact chain in both distance modes of the context. The reference
 * has no top-k by distance, so the order is ours: the distances that are
 * numbers first, ascending by value (-0.0 == 0.0), equal values by ascending
 * row; then the rows whose distance is a NaN, by ascending row (x86's NaN
 * bits). cnt_dev[q] (or NULL) = min(k, N); the slots past it hold row -1 and
 * distance 0.0. For k = 1 the result is lshkm_min_vector_dist's on every query
 * whose row 0 distance is not a NaN: that function's "NaN at row 0 wins" is the
 * reference loop's rule and is not reproduced here (a NaN comes last).
 * 1 <= k <= LSHKM_KNN_KMAX (one wave settles a query, a result slot per lane).
 * d <= 128 goes through the f32 MFMA screen of lshkm_min_vector_dist with its
 * bound: the rows are cut into disjoint groups, the
 * threshold of a query is the k-th smallest of its groups' smallest upper
 * bounds, and only the rows whose lower bound does not exceed it go to the
 * exact chain; d > 128, calls with fewer than k groups or real rows, and every
 * query the screen cannot decide (a poison query, more kept rows than the
 * capacity) take the exact scan over all rows. N < 2^31, nq < 2^31, d >= 1,
 * metric euclidean or cosine, row_dev and dist_dev not NULL, k in range: else
 * LSHKM_ERR_ARG, before any device work. N == 0: every slot empty; nq == 0 does
 * no device work. Returns after its workspace is free for the next call. */
#define LSHKM_KNN_KMAX 64
int lshkm_knn(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const float* Q_dev, int64_t nq, int metric, int k,
              int32_t* row_dev /*[nq][k]*/, double* dist_dev /*[nq][k]*/, int32_t* cnt_dev /*[nq] or NULL*/);
int lshkm_knn_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const double* Q_dev, int64_t nq, int metric,
                  int k, int32_t* row_dev, double* dist_dev, int32_t* cnt_dev);
/* The same over each query's own candidate vector X[cand_idx_dev[cand_ptr_dev[q]
 * .. cand_ptr_dev[q+1])] (lshkm_lsh_query's and lshkm_cube_query's CSR): the
 * tie-breaking key is the position in the list, cnt_dev[q] = min(k, the list's
 * length), row_dev holds dataset rows (cand_idx's values). A cand_ptr that
 * does not start at 0 or decreases, or an index outside [0, N), is
 * LSHKM_ERR_ARG (checked on the device before anything is written). */
int lshkm_knn_lists(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const float* Q_dev, int64_t nq, int metric,
                    int k, const int64_t* cand_ptr_dev /*[nq+1]*/, const int32_t* cand_idx_dev, int32_t* row_dev,
                    double* dist_dev, int32_t* cnt_dev);
int lshkm_knn_lists_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const double* Q_dev, int64_t nq,
                        int metric, int k, const int64_t* cand_ptr_dev, const int32_t* cand_idx_dev, int32_t* row_dev,
                        double* dist_dev, int32_t* cnt_dev);
/* get_top_N_recom (crypto_rec.hpp:305-325) over lshkm_p_closest's lists:
 * predicted scores of each user's unknown indexes (get_predicted_user_sim,
 * :280-302; unk_* = CSR of the ascending unknown indexes, std::set order),
 * sorted by the same quicksort, first n_top (0-padded like vector::resize).
 * x_mean_dev [N] / u_mean_dev [nq]: getKnownMean of the rows / users.
 * out_dev [nq][n_top]. */
int lshkm_top_n_recom(lshkm_ctx ctx, const double* X_dev, const double* x_mean_dev, int64_t N, int d,
                      const double* u_mean_dev, int64_t nq, const int64_t* unk_ptr_dev, const int32_t* unk_idx_dev,
                      const int32_t* nb_idx_dev, const double* nb_sim_dev, const int32_t* nb_cnt_dev, int P,
                      int n_top, int32_t* out_dev);

/* get_top_N_recom(neighbors, user, N) -- the 3-argument overload
 * (crypto_rec.hpp:327-345) -- as the clustering recommenders call it:
 * main.cpp:260-269 (Part A: user q's own cluster) and :353-373 (Part B: the
 * cluster of the user's nearest centroid, i.e. lshkm_lloyd_assign of the users
 * without the override). User q's neighbours are the members of cluster
 * ucl_dev[q], crows_dev[crow_dev[c] .. crow_dev[c+1]) in member order (what
 * lshkm_clusters returns: separate_clusters_from_input, utils.hpp:150-158);
 * similarities = cosineSimilarity(member, user) in that order (x87-exact,
 * cust_vector.hpp:158-174); predictions = get_predicted_user_sim over all of
 * them (:280-306; x_mean_dev [N] / u_mean_dev [nq] = getKnownMean, unk_* = CSR
 * of each user's ascending unknown indexes, values in [0, d)); the reference's
 * quicksort of the predictions (:234-277, ties / NaNs included); out_dev
 * [nq][n_top] = the first n_top unknown indexes, 0-padded like vector::resize.
 * Users whose cluster is empty get -1 in every slot: main.cpp skips them
 * (:262, :366). A ucl outside [0, K) is LSHKM_ERR_ARG (the reference indexes
 * clusters[ucl] unchecked; the same holds for the sharded entry points below). X_dev [N][d] pool rows and U_dev [nq][d]
 * users share the element type (for Part A pass the same rows twice). Counter
 * 7 counts the similarities the x87 chain decided. Bit-exact on any rows (the
 * norms' squares are glibc's pow(x, 2)). */
int lshkm_cluster_top_n(lshkm_ctx ctx, const float* X_dev, const double* x_mean_dev, int64_t N, int d,
                        const int64_t* crow_dev, const int32_t* crows_dev, int K, const float* U_dev,
                        const double* u_mean_dev, int64_t nq, const int32_t* ucl_dev, const int64_t* unk_ptr_dev,
                        const int32_t* unk_idx_dev, int n_top, int32_t* out_dev);
int lshkm_cluster_top_n_f64(lshkm_ctx ctx, const double* X_dev, const double* x_mean_dev, int64_t N, int d,
                            const int64_t* crow_dev, const int32_t* crows_dev, int K, const double* U_dev,
                            const double* u_mean_dev, int64_t nq, const int32_t* ucl_dev, const int64_t* unk_ptr_dev,
                            const int32_t* unk_idx_dev, int n_top, int32_t* out_dev);

/* The same over row shards (the C5 recommend step): a cluster's
 * members lie on every rank, in row order = rank order, and
 * get_predicted_user_sim's sums (crypto_rec.hpp:285-303) run over them in that
 * order -- so the sums pass from rank to rank (point-to-point, like the exact
 * k-means carry). Every rank holds the same nq query users (U_dev rows,
 * u_mean, ucl = their global cluster IDs, the unknown lists) and the CSR of
 * its own rows' clusters (lshkm_clusters of its assignment: local row ids).
 * lshkm_cluster_sims: each user's similarities to this rank's members of its
 *   cluster, the bulk of the work and independent of the other ranks:
 *   soff_dev [nq+1] <- offsets; sims_dev [cap] <- the similarities in member
 *   order when *total_host <= cap (call with sims_dev = NULL to size).
 * lshkm_cluster_chain: the prediction sums continued over this rank's members
 *   from the previous rank's carry (carry_* all NULL on rank 0): carry_main /
 *   main_out [total unknown indexes] (per unknown index, unk_ptr order),
 *   carry_abs / abs_out and carry_cnt / cnt_out [nq] (sum |sim|, members so
 *   far); send the outputs to the next rank. The last rank passes out_dev
 *   [nq][n_top] instead (main_out etc. may be NULL): the predictions, the
 *   quicksort and the first n_top as lshkm_cluster_top_n, -1 for users whose
 *   cluster is empty on every rank. Chained over the ranks in row order this is
 *   lshkm_cluster_top_n over the concatenated rows, bit for bit. */
int lshkm_cluster_sims(lshkm_ctx ctx, const float* X_dev, int64_t N, int d, const int64_t* crow_dev,
                       const int32_t* crows_dev, int K, const float* U_dev, int64_t nq, const int32_t* ucl_dev,
                       const int64_t* unk_ptr_dev, int64_t* soff_dev, double* sims_dev, int64_t cap,
                       int64_t* total_host);
int lshkm_cluster_sims_f64(lshkm_ctx ctx, const double* X_dev, int64_t N, int d, const int64_t* crow_dev,
                           const int32_t* crows_dev, int K, const double* U_dev, int64_t nq, const int32_t* ucl_dev,
                           const int64_t* unk_ptr_dev, int64_t* soff_dev, double* sims_dev, int64_t cap,
                           int64_t* total_host);
int lshkm_cluster_chain(lshkm_ctx ctx, const float* X_dev, const double* x_mean_dev, int64_t N, int d,
                        const int64_t* crow_dev, const int32_t* crows_dev, int K, int64_t nq, const int32_t* ucl_dev,
                        const double* u_mean_dev, const int64_t* unk_ptr_dev, const int32_t* unk_idx_dev,
                        const int64_t* soff_dev, const double* sims_dev, const double* carry_main_dev,
                        const double* carry_abs_dev, const int64_t* carry_cnt_dev, double* main_out_dev,
                        double* abs_out_dev, int64_t* cnt_out_dev, int n_top, int32_t* out_dev);
int lshkm_cluster_chain_f64(lshkm_ctx ctx, const double* X_dev, const double* x_mean_dev, int64_t N, int d,
                            const int64_t* crow_dev, const int32_t* crows_dev, int K, int64_t nq,
                            const int32_t* ucl_dev, const double* u_mean_dev, const int64_t* unk_ptr_dev,
                            const int32_t* unk_idx_dev, const int64_t* soff_dev, const double* sims_dev,
                            const double* carry_main_dev, const double* carry_abs_dev, const int64_t* carry_cnt_dev,
                            double* main_out_dev, double* abs_out_dev, int64_t* cnt_out_dev, int n_top,
                            int32_t* out_dev);

/* The terms form of the same two phases (what sharding.recommend_sharded and
 * lshkm_cluster_top_n run): phase 1 also forms get_predicted_user_sim's terms
 * sim_i * (x_i[index] - mean_i) (crypto_rec.hpp:296) while the member rows are
 * on chip, so the rank-to-rank chain reads no rows.
 * lshkm_cluster_terms: soff_dev / toff_dev [nq+1] <- the offsets of each user's
 *   similarities (member order) and terms (member-major: toff[q] + i * m_q + e,
 *   m_q = the user's unknown indexes); sims_dev [cap] / terms_dev [tcap] filled when the totals
 *   (*total_host, *tterms_host) fit (NULL to size). Rows of d * sizeof(elem) a
 *   multiple of 8 B and at most 1016 B (else LSHKM_ERR_ARG: the form above).
 * lshkm_cluster_chain_terms: lshkm_cluster_chain from them (same carry and
 *   outputs). */
int lshkm_cluster_terms(lshkm_ctx ctx, const float* X_dev, const double* x_mean_dev, int64_t N, int d,
                        const int64_t* crow_dev, const int32_t* crows_dev, int K, const float* U_dev, int64_t nq,
                        const int32_t* ucl_dev, const int64_t* unk_ptr_dev, const int32_t* unk_idx_dev,
                        int64_t* soff_dev, int64_t* toff_dev, double* sims_dev, double* terms_dev, int64_t cap,
                        int64_t tcap, int64_t* total_host, int64_t* tterms_host);
int lshkm_cluster_terms_f64(lshkm_ctx ctx, const double* X_dev, const double* x_mean_dev, int64_t N, int d,
                            const int64_t* crow_dev, const int32_t* crows_dev, int K, const double* U_dev, int64_t nq,
                            const int32_t* ucl_dev, const int64_t* unk_ptr_dev, const int32_t* unk_idx_dev,
                            int64_t* soff_dev, int64_t* toff_dev, double* sims_dev, double* terms_dev, int64_t cap,
                            int64_t tcap, int64_t* total_host, int64_t* tterms_host);
int lshkm_cluster_chain_terms(lshkm_ctx ctx, int64_t nq, const double* u_mean_dev, const int64_t* unk_ptr_dev,
                              const int32_t* unk_idx_dev, const int64_t* soff_dev, const int64_t* toff_dev,
                              const double* sims_dev, const double* terms_dev, const double* carry_main_dev,
                              const double* carry_abs_dev, const int64_t* carry_cnt_dev, double* main_out_dev,
                              double* abs_out_dev, int64_t* cnt_out_dev, int n_top, int32_t* out_dev);
/* 1 when rows of d values (fp64 when f64 != 0, else fp32) take the terms form
 * (lshkm_cluster_terms accepts them), else 0 (lshkm_cluster_sims +
 * lshkm_cluster_chain): the rule lshkm_cluster_top_n itself routes by. Needs
 * no context. */
int lshkm_cluster_terms_supported(int d, int f64);

/* ------------------------------------------------ recommender validation
 * lsh_rec_10_fold_validation_A (main.cpp:393-437, called at :180-183) and the
 * helpers it sits on. The reference seeds srand with time(0) and its LSH
 * generators with the clock: both are explicit seeds here. rand() is glibc's
 * (its additive-feedback generator after srand(seed)), restated in the library:
 * the process-global srand / rand are never called.
 *
 * split_to_10 (crypto_rec.hpp:348-367), host only: srand(seed), F = N / 10;
 * for each of 10 folds, F times: rand() % remaining.size(), that element taken
 * and erased. rows_host [10][F]: the users (indexes into the caller's vector)
 * in fold order; the last N % 10 users occur nowhere. An order-statistic tree
 * replaces the reference's O(N) erase. 0 <= N < 2^31. */
int lshkm_cv_split10(uint64_t seed, int64_t N, int32_t* rows_host /*[10][N/10]*/);
/* The first `per` values of rand() after srand(seed_host[i]), i < n, host only:
 * draw_host [n][per] (per = 1: hide_one_score's draw, crypto_rec.hpp:410-411). */
int lshkm_cv_draws(const uint64_t* seed_host, int64_t n, int64_t per, int32_t* draw_host);
/* hide_one_score (crypto_rec.hpp:393-449) for N users at once. X_dev [N][d]
 * with means x_mean_dev [N]; unk_* = the CSR of each user's ascending unknown
 * indexes (as lshkm_top_n_recom takes it); draw_dev [N]: each user's rand()
 * value (lshkm_cv_draws). Per user: known_count = d - |unknown| < 2 returns
 * false with nothing changed (:405-406); hide_index = draw % known_count is
 * used directly as a dimension index (:411-412: it may land on an unknown
 * index); old_score is read before the unknown entries are set to 0
 * (:412-416); new_mean = the sequential sum from 0.0 of the other d - 1
 * entries in index order, divided by d - 1 (:419-436); when all of them are 0
 * the function returns false after the zeroing (:432-433).
 * H_dev [N][d] / h_mean_dev [N]: the user as the function leaves it (unchanged;
 * zeroed with the old mean; or hidden with the new mean); hide_idx_dev [N]:
 * the hidden index, the user's one unknown index afterwards, or -1 where the
 * function returned false; old_dev [N]: *old_score (0.0, main.cpp:409's initial
 * value, where known_count < 2). */
int lshkm_cv_hide(lshkm_ctx ctx, const double* X_dev, const double* x_mean_dev, int64_t N, int d,
                  const int64_t* unk_ptr_dev, const int32_t* unk_idx_dev, const int32_t* draw_dev, double* H_dev,
                  double* h_mean_dev, int32_t* hide_idx_dev, double* old_dev);
/* merge_except_for (crypto_rec.hpp:370-390) applied to a filled query result
 * over all folds' rows: drops the members in [lo, hi) from every query's
 * ascending list. in_ptr_dev [nq+1] / in_idx_dev: lshkm_lsh_query's output;
 * out_ptr_dev [nq+1] <- the new offsets; out_idx_dev (NULL: offsets only; else
 * room for in_ptr[nq] rows, a different buffer than in_idx_dev) <- the kept
 * members in their order. */
int lshkm_cv_exclude(lshkm_ctx ctx, const int64_t* in_ptr_dev, const int32_t* in_idx_dev, int64_t nq, int32_t lo,
                     int32_t hi, int64_t* out_ptr_dev, int32_t* out_idx_dev);
/* get_predicted_user_sim (crypto_rec.hpp:280-306) over lshkm_p_closest's
 * lists, as values: pred_dev[e] for entry e of the unknown-index CSR
 * (unk_ptr_dev [nq+1] with unk_ptr[0] = 0, unk_idx_dev) = main_sum / abs_sum +
 * u_mean, both sums over the user's kept neighbours in their sorted order
 * (:289-297) -- the sums lshkm_top_n_recom sorts by. No neighbour or all
 * similarities 0 gives 0 / 0: NaNs are x86's default NaN; a NaN similarity
 * comes through with its own sign, as x86 hands an operand NaN on. */
int lshkm_predicted_scores(lshkm_ctx ctx, const double* X_dev, const double* x_mean_dev, int64_t N, int d,
                           const double* u_mean_dev, int64_t nq, const int64_t* unk_ptr_dev, const int32_t* unk_idx_dev,
                           const int32_t* nb_idx_dev, const double* nb_sim_dev, const int32_t* nb_cnt_dev, int P,
                           double* pred_dev);
/* One fold's ordered error sum (main.cpp:413-425) over its nq held-out users in
 * fold order: user q counts when hide_idx_dev[q] >= 0 and its neighbour list
 * nb_ptr_dev[q] .. nb_ptr_dev[q+1] is not empty; k_sum = k_sum + fabs(old_dev[q]
 * - pred_dev[q]), one sequential chain from 0.0 (no atomics, no tree).
 * *k_sum_dev / *count_dev: k_sum and calc_user_num; err_dev [nq] (may be NULL):
 * each user's error, -1.0 for the skipped ones. A NaN is x86's: fabs of the
 * default NaN (0x7FF8...), kept by every later add. */
int lshkm_cv_fold_sum(lshkm_ctx ctx, int64_t nq, const int32_t* hide_idx_dev, const double* old_dev,
                      const double* pred_dev, const int64_t* nb_ptr_dev, double* err_dev, double* k_sum_dev,
                      int64_t* count_dev);
/* lsh_rec_10_fold_validation_A (main.cpp:393-437): the 10-fold mean absolute
 * error of the LSH recommender over users X_dev [N][d] (means x_mean_dev,
 * unknown-index CSR unk_*; all left unmodified, as the reference splits by
 * value). split_seed: split_to_10's srand; hide_seed, or hide_seeds_host [N]
 * per user when not NULL: hide_one_score's srand (the reference re-seeds with
 * the wall-clock second on every call); lsh_seeds_host [10]: fold i's
 * create_LSH_hashtables (lshkm_params_lsh_cosine / _euclidean; euclidean with
 * nb = pool size / lsh_bucket_div, main.cpp:402-404).
 * Fold i: the pool is every other fold -- folds < i in their hidden form, as
 * the earlier loop bodies left them (:407-410 mutate in place), folds > i
 * untouched, in fold order; each held-out user for which hide_one_score
 * returned true and whose filtered union (lsh_cube.hpp:93-106) is not empty
 * adds fabs(old_score - prediction at the hidden index) to k_sum in fold order
 * (:413-424). NaNs are not filtered (a zero pool row gives a NaN k_sum).
 * *mae_host = sum over the folds with users of k_sum / calc_user_num, / 10
 * (:428-434); fold_sum_host / fold_cnt_host [10] (may be NULL): k_sum and
 * calc_user_num; err_dev [10 * (N / 10)] (may be NULL): every user's error in
 * split order, -1.0 for the skipped ones.
 * N < 10: 0.0, no device work (every fold is empty). P < 1, d < 1,
 * lsh_bucket_div < 1 or a euclidean nb of 0 (the reference divides by zero):
 * LSHKM_ERR_ARG. Returns after the result is on the host. */
int lshkm_lsh_validate10(lshkm_ctx ctx, const double* X_dev, const double* x_mean_dev, int64_t N, int d,
                         const int64_t* unk_ptr_dev, const int32_t* unk_idx_dev, int metric, int k, int L,
                         int lsh_bucket_div, float w, int P, uint64_t split_seed, uint64_t hide_seed,
                         const uint64_t* hide_seeds_host /*[N] or NULL*/, const uint64_t* lsh_seeds_host /*[10]*/,
                         double* mae_host, double* fold_sum_host /*[10]*/, int64_t* fold_cnt_host /*[10]*/,
                         double* err_dev /*[10 * (N / 10)] or NULL*/);

/* ------------------------------------------------------------ input formats
 * Host only (no device needed). VectorReader<double>::read
 * (vector_reader.hpp:54-85): lines 1..strt_line-1 kept as metadata, then one
 * vector per line: '\r' removed, ID = text before the first delimiter, values
 * = std::stod of each delimiter-separated token (getline semantics). A token
 * std::stod would throw on fails the call. threads <= 0: all hardware threads. */
int lshkm_vectors_read(const char* path, char delimiter, int strt_line, int threads, lshkm_vectors* out);
/* n rows, d = values of row 0, id_bytes = total ID length, ragged = rows of
 * different lengths, fp32_exact = every value is an fp32 value (the hot
 * path's storage contract), n_meta = metadata lines. Any pointer may be NULL. */
int lshkm_vectors_info(lshkm_vectors v, int64_t* n, int* d, int64_t* id_bytes, int* ragged, int* fp32_exact,
                       int* n_meta);
/* Row-major values: X64_host [n][d] and/or X32_host [n][d] (either may be NULL). */
int lshkm_vectors_values(lshkm_vectors v, double* X64_host, float* X32_host);
/* IDs: bytes_host [id_bytes] concatenated, offsets_host [n+1]. */
int lshkm_vectors_ids(lshkm_vectors v, char* bytes_host, int64_t* offsets_host);
/* getMetaLine(index) (vector_reader.hpp:91-96): "" past the saved lines. */
int lshkm_vectors_meta(lshkm_vectors v, int index, char* buf, int64_t cap, int64_t* len);
int lshkm_vectors_free(lshkm_vectors v);

/* cluster.conf: file_to_args(path, ' ') + ArgParser::getFlagValue — the token
 * after the first occurrence of key (*found = 0: absent, or last token). */
int lshkm_config_value(const char* path, const char* key, char* buf, int64_t cap, int* found);
/* get_config (main.cpp:512-554): the reference's defaults (main.cpp:50-63),
 * then every key present; csv_delimiter is an ASCII code, proj_2_csv_delimiter
 * the first character. Fails where the reference's stoi / stod would throw. */
typedef struct lshkm_config {
    char proj_2_input[1024];
    char proj_2_csv_delimiter;
    int proj_2_cluster_num;
    int cluster_num;
    int has_cluster_num;      /* 0: the reference would ask on stdin */
    int k, L, lsh_bucket_div;
    double euclidean_h_w;
    char csv_delimiter;
    int max_algo_iterations;
    double min_dist_kmeans;
    char lexicon_file[1024];
    char query_file[1024];
} lshkm_config;
int lshkm_config_load(const char* path, lshkm_config* out);

/* ------------------------------------------------- tweets and user vectors
 * main.cpp:121-137: the tweet file, the lexicon and the coin file become
 * user_vectors (tweets_to_user_vectors, crypto_rec.hpp:78-140) and
 * fake_user_vectors (clusters_to_user_vectors, crypto_rec.hpp:143-210).
 *
 * Host: the formats and the visiting order. file_to_str_vectors (utils.cpp:72-127):
 * the tweet file's first line sets P from its second token when it has one
 * (else P = 1, main.cpp:120); every later line, a trailing '\r' dropped, is
 * split on the delimiter: user ID, tweet ID, words. The coin file (query_path)
 * is one coin per line, every token a variation. file_to_lexicon
 * (utils.cpp:130-147): word<delim>score through std::stof, the first occurrence
 * of a word wins. Tweet::Tweet (tweet.cpp:11-42): a word of the lexicon adds its
 * float score to a double total in word order; any other word is compared with
 * every variation of every coin and the matching coin indexes form a std::set;
 * score = total / sqrt(total * total + 15). The tweet map (main.cpp:128-132)
 * keeps the first tweet of a duplicated ID. Tweets are numbered in the
 * iteration order of that std::unordered_map, users in the iteration order of
 * tweets_to_user_vectors' user_map (crypto_rec.hpp:80-95, :107): both are
 * libstdc++'s, reproduced with the same container and insertion sequence.
 * Where the reference has undefined behaviour -- a tweet line or a lexicon
 * line with fewer than two tokens, a score or a P that std::stof / std::stoi
 * rejects -- and where a file cannot be opened (the reference goes on with an
 * empty table), the call returns LSHKM_ERR_ARG, lshkm_last_error names file
 * and line, and nothing is built. threads <= 0: the hardware's. */
int lshkm_tweets_read(const char* input_path, const char* lexicon_path, const char* query_path, char delimiter,
                      int threads, lshkm_tweets* out);
/* P, the number of distinct tweet IDs, of distinct user IDs, of coin-file
 * lines (crypto_num, main.cpp:135), of (tweet, coin) mentions, and the total
 * byte lengths of the tweet and user IDs. Any pointer may be NULL. */
int lshkm_tweets_info(lshkm_tweets t, int* P, int64_t* n_tweets, int64_t* n_users, int* crypto_num, int64_t* mentions,
                      int64_t* id_bytes, int64_t* user_id_bytes);
/* The tweets in map order: score_host [T] (getSentimentScore), ci_ptr_host
 * [T+1] / ci_idx_host [mentions] (getCryptoIndexes: ascending, distinct),
 * user_of_host [T] (the user's slot in user_map order). Any may be NULL. */
int lshkm_tweets_table(lshkm_tweets t, double* score_host, int64_t* ci_ptr_host, int32_t* ci_idx_host,
                       int32_t* user_of_host);
/* Tweet IDs in map order / user IDs in user_map order: bytes concatenated, offsets [n+1]. */
int lshkm_tweets_ids(lshkm_tweets t, char* bytes_host, int64_t* offsets_host);
int lshkm_tweets_user_ids(lshkm_tweets t, char* bytes_host, int64_t* offsets_host);
/* tweets.count(vec.getId()) (crypto_rec.hpp:159) for n row IDs (lshkm_vectors_ids'
 * layout): tweet_of_row_host[i] = the tweet's number, or -1. */
int lshkm_tweets_match(lshkm_tweets t, const char* id_bytes, const int64_t* id_offsets, int64_t n,
                       int32_t* tweet_of_row_host);
/* The printers' host side (main.cpp:557-569, :151-173). The name
 * print_recommendations prints for every line of the coin file (query_crypto):
 * field name_index where the line has more than name_index fields, else field 0
 * (main.cpp:563-566; the program passes 4); a line without any field, where the
 * reference reads out of bounds, has the empty name. bytes_host concatenated
 * (NULL: the offsets alone, for the size), offsets_host [crypto_num + 1]. */
int lshkm_tweets_coin_names(lshkm_tweets t, int name_index, char* bytes_host, int64_t* offsets_host);
/* One block of the program's output file: the title line (main.cpp:151, :197,
 * :242, :336), then for every user q with skip_host[q] == 0 (NULL: none
 * skipped), in order, print_recommendations' line (main.cpp:557-569) -- the ID,
 * then " " + the name of coin top_host[q][j] for j < n_top, then "\n" -- and
 * "Execution Time: <elapsed_ms>" (main.cpp:173), every line ended by '\n'.
 * append == 0 truncates path (the ofstream of main.cpp:140), else the block is
 * added at its end. get_top_N_recom's resize(N) padding arrives as index 0 and
 * prints coin 0's name, as in the reference. An index outside [0, crypto_num)
 * of a user that is not skipped is LSHKM_ERR_ARG, found before the file is
 * opened; a path that cannot be opened or written is LSHKM_ERR_ARG too. */
int lshkm_recom_write(lshkm_tweets t, int name_index, const char* path, int append, const char* title,
                      const char* user_id_bytes, const int64_t* user_id_offsets, int64_t nq, const int32_t* top_host,
                      int n_top, const uint8_t* skip_host, int64_t elapsed_ms);
int lshkm_tweets_free(lshkm_tweets t);

/* The update loop both functions share (crypto_rec.hpp:97-102, :166-171) over a
 * list of visits v = 0..V-1 in the reference's loop order: tweet tw_dev[v]
 * updates group grp_dev[v] (a user slot, or vec.getCluster()); tw or grp == -1:
 * the visit is skipped (a vector that is no tweet, :159). For every (g, j):
 * sum_dev[g][j] = the chain s = s + score over the visits of g whose tweet lists
 * coin j and whose score is > 0, in visit order, from carry_sum_dev[g][j] (NULL:
 * +0.0): the reference's fp64 value bit for bit (a NaN, zero or negative score
 * adds nothing, +inf is added); known_dev[g][j] = the carry's flag OR "some
 * visit of g lists j", whatever the score. With the carry, contiguous shards of
 * the visit list passed in order give the single pass's result. sum_dev /
 * known_dev may alias the carry. No floating-point atomics: the incidences are
 * ordered by (g, j) with the stable scatter and every chain is summed in order.
 * A tw outside [-1, T), a grp outside [-1, G), a ci_idx outside [0, C) or a
 * decreasing ci_ptr: LSHKM_ERR_ARG (checked on the device before anything is
 * written). G * C >= 2^31, V >= 2^31 or 2^31 incidences: LSHKM_ERR_UNSUPPORTED.
 * Returns after the stream has drained. */
int lshkm_user_sums(lshkm_ctx ctx, const int32_t* tw_dev, const int32_t* grp_dev, int64_t V, const double* score_dev,
                    const int64_t* ci_ptr_dev, const int32_t* ci_idx_dev, int64_t T, int64_t G, int C,
                    const double* carry_sum_dev, const uint8_t* carry_known_dev, double* sum_dev /*[G][C]*/,
                    uint8_t* known_dev /*[G][C]*/);
/* Finishing a user (crypto_rec.hpp:107-137, :177-207), for every group g and i
 * ascending: an unknown i (flag 0) joins the unknown set, a known i does sum =
 * sum + v[i]; a group whose every v[i] == 0 is dropped; else mean = sum /
 * known_number and every unknown entry holds the mean. The kept groups are
 * compacted in group order: U_dev [n_kept][C], mean_dev [n_kept], unk_ptr_dev
 * [n_kept+1] / unk_idx_dev (ascending), src_dev[i] = the group of kept row i --
 * the U / u_mean / unk_ptr / unk_idx (X / x_mean) arguments of
 * lshkm_top_n_recom, lshkm_cluster_top_n, lshkm_lsh_p_closest and
 * lshkm_lsh_validate10. Rows past n_kept are not written. G * C >= 2^31:
 * LSHKM_ERR_UNSUPPORTED. Returns after *n_kept_host is on the host. */
int lshkm_user_finish(lshkm_ctx ctx, const double* sum_dev, const uint8_t* known_dev, int64_t G, int C, double* U_dev,
                      double* mean_dev, int64_t* unk_ptr_dev, int32_t* unk_idx_dev, int32_t* src_dev,
                      int64_t* n_kept_host);

/* ------------------------------------------------------------ synthetic data */
/* include/lshkm_synth.h generator, rows [row0, row0+rows) into X_dev. */
int lshkm_synth(lshkm_ctx ctx, uint64_t seed, int64_t row0, int64_t rows, int d, float* X_dev);
/* The "normal" generator of include/lshkm_synth.h (Irwin-Hall(12), full fp32
 * mantissas; SURVEY.md §8d's N(0,1) rows), rows [row0, row0+rows) into X_dev. */
int lshkm_synth_normal(lshkm_ctx ctx, uint64_t seed, int64_t row0, int64_t rows, int d, float* X_dev);

#ifdef __cplusplus
}
#endif
#endif /* LSHKM_H */
