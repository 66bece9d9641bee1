// kmeanspp.hip — k-means++ seeding (k_means_pp, lib/clustering_phases/
// initialization.hpp:71-156) on gfx950, bit-exact with the reference.
//
// Per new centroid i = 1..K-1 the reference
//   (1) takes every row's min distance to centroids 0..i-1 (strict '<' after
//       the -1 sentinel, :88-110; its ID-keyed cache only memoises),
//   (2) the max of those minima (strict '>' from 0, :112-113),
//   (3) overwrites them with (min/max)^2 and prefix-sums them in row order,
//       in fp64 (:118-125),
//   (4) draws uniform_real<double>(0, total) and binary-searches (:127-149).
// (1) is incremental here: one exact distance per row per centroid
// (kpp_dist_kernel), the running minimum kept in HBM. (4) needs only the
// engine's canonical draws, which do not depend on the data, so the host draws
// them all up front and the whole seeding runs on the stream with no host
// round trip.
//
// (3) is a strictly sequential fp64 chain s_m = RN(s_{m-1} + q_m) over N rows,
// reproduced exactly, in parallel, as an integer prefix sum inside each binade
// of s: kpp_chain.h states that arithmetic and every rounding decision (checked
// on the host against the plain chain), kpp_layout.h the workspace. The wave-
// parallel forms are here. Rows are cut into chunks of KPP_CHUNK:
//   kpp_scan_kernel         the max of the minima; approximate chunk starts
//                           (the distance pass's sum m^2 per 256 rows / max^2)
//   kpp_chunk_units_kernel  each chunk's record in the binade guessed from its
//                           approximate start, its prefix arrays if it has any
//   kpp_chain_kernel        one wave walks the chunks with the EXACT running s
//                           (kpp_walk), 512 chunks per wave-wide integer scan;
//                           then the draw and the reference's binary search,
//                           the prefix sums formed only for the draw's chunk.
//
// Over contiguous row shards (lshkm_kpp_shard_*) the same device code runs per
// shard with the host between the steps: a later row needs from the earlier
// ones only the global max and the exact running s, and the chain's value does
// not depend on where the chunks are cut. kpp_fold_kernel leaves the shard's max
// and sum m^2 for the exchange; kpp_starts_kernel takes the global max and the
// approximate sum before the shard; kpp_chain_shard_kernel walks from the previous
// shard's s (no draw); kpp_pick_shard_kernel searches for the host's draw.
#include "common.h"
#include "kernels.h"
#include "exact.h"
#include "kpp_layout.h"

namespace lshkm {

constexpr int KPP_THREADS = KPP_GROUP;         // a thread per row of a group; a chunk = 2 rows per thread

// q_m = (min_m / max)^2, as :121-124 (two roundings).
__device__ inline double kpp_q(double m, double mx) {
    const double t = __ddiv_rn(m, mx);
    return __dmul_rn(t, t);
}

// Wave-level helpers of the exact walk (one wave, every lane active): an inclusive
// int64 scan by DPP row shifts inside each 16-lane row plus the row totals by
// readlane (no LDS round trips, unlike __shfl_up), and reads of a uniform lane.
template <int K>   // row_shr:K (0x110 + K); lanes without a source read 0 (bound_ctrl)
__device__ inline int64_t dpp_shr64(int64_t v) {
    const int lo = (int)(uint32_t)(uint64_t)v, hi = (int)(uint32_t)((uint64_t)v >> 32);
    const int rl = __builtin_amdgcn_update_dpp(0, lo, 0x110 + K, 0xF, 0xF, true);
    const int rh = __builtin_amdgcn_update_dpp(0, hi, 0x110 + K, 0xF, 0xF, true);
    return (int64_t)(((uint64_t)(uint32_t)rh << 32) | (uint32_t)rl);
}
__device__ inline int64_t readlane64(int64_t v, int l) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, l);
    const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ inline int64_t wave_incl_scan64(int64_t v, int lane) {
    v += dpp_shr64<1>(v);
    v += dpp_shr64<2>(v);
    v += dpp_shr64<4>(v);
    v += dpp_shr64<8>(v);
    const int64_t t0 = readlane64(v, 15), t1 = readlane64(v, 31), t2 = readlane64(v, 47);
    const int row = lane >> 4;
    return v + (row > 0 ? t0 : 0) + (row > 1 ? t1 : 0) + (row > 2 ? t2 : 0);
}

// ------------------------------------------------------------- (1) + (2)
// Distances of every row to the newest centroid (row chosen[it-1] of X, or the
// [d] row cext of the rows' type when it is given: a shard, whose newest
// centroid usually lies on another rank), the running minimum, and the max of
// the minima (positive doubles order as their bit patterns; the reference's max
// starts at 0 with '>', so only m > 0 count).
// A block owns 256 rows (one per thread) and streams them through LDS in
// slices of KPP_DJ dims, loaded coalesced (consecutive lanes, consecutive
// floats of a row); each thread then accumulates its row in dim order, exactly
// as exact.h. The centroid row is read with uniform (scalar) loads.
// VEC (d % 32 == 0): each slice is 8 float4 per thread, all in flight at
// once, and the next slice's loads are issued before the current one is
// consumed (register double buffer).
constexpr int KPP_DJ = 32;
constexpr int KPP_V4 = KPP_THREADS * KPP_DJ / 4 / KPP_THREADS;   // float4 per thread per slice (8)

// The max of the minima: each block writes its own (positive doubles order as
// their bit patterns; 0 when it has none) for kpp_fold_max -- one global atomic
// per wave on a single word serialised at ~12 ns each (~0.19 ms at N = 1M).
__device__ inline void kpp_block_max(double best, unsigned long long* __restrict__ bmax) {
    __shared__ double wbest[KPP_THREADS / 64];
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(best, off);
        if (o > best) best = o;
    }
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = 0.0;
        for (int w = 0; w < KPP_THREADS / 64; w++)
            if (wbest[w] > b) b = wbest[w];
        bmax[blockIdx.x] = (unsigned long long)__double_as_longlong(b);
    }
}

// Sum of the block's m^2 (any order: only the chunk guesses use it) for its
// 256-row group g. Every thread of the block calls it.
__device__ inline void kpp_group_sum(double v, double* __restrict__ gsum, int64_t g) {
    __shared__ double wsum[KPP_THREADS / 64];
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < KPP_THREADS / 64; w++) t += wsum[w];
        gsum[g] = t;
    }
    __syncthreads();
}

// Row n's distance dd to the newest centroid -> its running minimum (the
// earlier value unless dd is strictly smaller) -> mind[n] and the thread's max.
__device__ inline double kpp_take_min(double dd, int it, double* __restrict__ mind, int64_t n, double& best) {
    double m = dd;
    if (it > 1) {
        const double prev = mind[n];
        if (!(dd < prev)) m = prev;
    }
    mind[n] = m;
    if (m > best) best = m;
    return m;
}

// TX: fp32 or fp64 rows (VEC only for fp32).
template <int METRIC, bool VEC, typename TX>
__global__ __launch_bounds__(KPP_THREADS) void kpp_dist_kernel(
    const TX* __restrict__ X, int64_t N, int d, const int32_t* __restrict__ chosen, const TX* __restrict__ cext, int it,
    double* __restrict__ mind, unsigned long long* __restrict__ bmax, double* __restrict__ gsum) {
    static_assert(!VEC || sizeof(TX) == 4, "the float4 form reads fp32 rows");
    constexpr int DJ = sizeof(TX) == 4 ? KPP_DJ : KPP_DJ / 2;     // tile <= 34 KiB either way
    __shared__ TX tile[KPP_THREADS][DJ + 1];
    __shared__ double sqs[METRIC == 0 ? KPP_THREADS / 64 : 1][64 * 8];   // gp_sq_wave: 64 * 8 per wave
    double* sqb = sqs[METRIC == 0 ? threadIdx.x >> 6 : 0];
    // the newest centroid's row, widened to fp64 once per block (LDS broadcast
    // reads in the chain instead of a uniform global load per dim)
    extern __shared__ __attribute__((aligned(8))) char kpp_dyn[];
    TX* cs = reinterpret_cast<TX*>(kpp_dyn);            // [d] (dynamic)
    const TX* __restrict__ c = cext ? cext : X + (int64_t)chosen[it - 1] * d;
    for (int j = threadIdx.x; j < d; j += KPP_THREADS) cs[j] = c[j];
    __syncthreads();
    double cb = 0.0;                                    // cosine: sum c^2 (uniform)
    if (METRIC == 1)
        for (int j = 0; j < d; j++) {
            const double cj = (double)cs[j];
            cb = __dadd_rn(cb, sq_of<TX>(cj));
        }
    double best = 0.0;
    for (int64_t row0 = (int64_t)blockIdx.x * KPP_THREADS; row0 < N; row0 += (int64_t)gridDim.x * KPP_THREADS) {
        const int64_t n = row0 + threadIdx.x;
        const int rows = (int)(N - row0 < KPP_THREADS ? N - row0 : KPP_THREADS);
        double acc = 0.0, a = 0.0;
        X87acc ip;
        ip.init();
        float4 pf[KPP_V4];
        if (VEC) {
#pragma unroll
            for (int k = 0; k < KPP_V4; k++) {
                const int idx = k * KPP_THREADS + threadIdx.x, r = idx >> 3, part = idx & 7;
                if (r < rows) pf[k] = *reinterpret_cast<const float4*>(X + (row0 + r) * d + part * 4);
            }
        }
        for (int j0 = 0; j0 < d; j0 += DJ) {
            const int dj = d - j0 < DJ ? d - j0 : DJ;
            __syncthreads();
            if (VEC) {
#pragma unroll
                for (int k = 0; k < KPP_V4; k++) {
                    const int idx = k * KPP_THREADS + threadIdx.x, r = idx >> 3, part = idx & 7;
                    if (r < rows) {
                        tile[r][part * 4 + 0] = pf[k].x;
                        tile[r][part * 4 + 1] = pf[k].y;
                        tile[r][part * 4 + 2] = pf[k].z;
                        tile[r][part * 4 + 3] = pf[k].w;
                    }
                }
            } else {
#pragma unroll 4
                for (int e = threadIdx.x; e < KPP_THREADS * DJ; e += KPP_THREADS) {
                    const int r = e / DJ, jj = e % DJ;
                    if (r < rows && jj < dj) tile[r][jj] = X[(row0 + r) * d + j0 + jj];
                }
            }
            __syncthreads();
            if (VEC && j0 + DJ < d) {
#pragma unroll
                for (int k = 0; k < KPP_V4; k++) {
                    const int idx = k * KPP_THREADS + threadIdx.x, r = idx >> 3, part = idx & 7;
                    if (r < rows)
                        pf[k] = *reinterpret_cast<const float4*>(X + (row0 + r) * d + j0 + DJ + part * 4);
                }
            }
            if (METRIC == 0) {
                // the whole block (rows past N too: their sums are dropped), the
                // squares through gp_sq_wave (glibc's pow batched over the wave)
                int jj = 0;
#pragma unroll 1
                for (; jj + 8 <= dj; jj += 8) {
                    double df[8], p[8];
#pragma unroll
                    for (int q = 0; q < 8; q++)
                        df[q] = __dsub_rn((double)tile[threadIdx.x][jj + q], (double)cs[j0 + jj + q]);
                    gp_sq_wave<8, sizeof(TX) == 8>(df, p, sqb);
#pragma unroll
                    for (int q = 0; q < 8; q++) acc = __dadd_rn(acc, p[q]);
                }
#pragma unroll 1
                for (; jj < dj; jj++) {
                    const double df[1] = {__dsub_rn((double)tile[threadIdx.x][jj], (double)cs[j0 + jj])};
                    double p[1];
                    gp_sq_wave<1, sizeof(TX) == 8>(df, p, sqb);
                    acc = __dadd_rn(acc, p[0]);
                }
            } else if (n < N) {
#pragma unroll 8
                for (int jj = 0; jj < dj; jj++) {
                    const double xj = (double)tile[threadIdx.x][jj];
                    const double cj = (double)cs[j0 + jj];
                    ip.add(__dmul_rn(xj, cj));
                    a = __dadd_rn(a, sq_of<TX>(xj));
                }
            }
        }
        double m = 0.0;
        if (n < N) {
            const double dd = METRIC == 0 ? sqrt(acc) : one_minus(x87_quot(ip.value(), __dmul_rn(sqrt(a), sqrt(cb))));
            m = kpp_take_min(dd, it, mind, n, best);
        }
        kpp_group_sum(m * m, gsum, row0 / KPP_THREADS);
    }
    kpp_block_max(best, bmax);
}

// Euclidean on fp32 rows with d % 32 == 0 (16-B aligned rows): each wave takes
// 64 consecutive rows and reads them 16 dims at a time as 16-B pieces, four
// lanes per row's 64 contiguous bytes (a row per lane touched 64 lines per
// load instruction), transposed through LDS with the next step's loads in
// flight; the squares go through gp_sq_wave (glibc's pow batched over the
// wave). The centroid row is an LDS broadcast. Same exact-order chain as above.
constexpr int KR_S = 20;                                 // LDS row stride of the transpose (floats)
__global__ __launch_bounds__(KPP_THREADS) void kpp_dist_reg_kernel(
    const float* __restrict__ X, int64_t N, int d, const int32_t* __restrict__ chosen, const float* __restrict__ cext,
    int it, double* __restrict__ mind, unsigned long long* __restrict__ bmax, double* __restrict__ gsum) {
    extern __shared__ __attribute__((aligned(8))) char kpp_dyn2[];
    float* cs = reinterpret_cast<float*>(kpp_dyn2);     // [d]
    __shared__ double sqs[KPP_THREADS / 64][64 * 16];   // gp_sq_wave: 64 * 16 per wave
    __shared__ __attribute__((aligned(16))) float trs[KPP_THREADS / 64][64 * KR_S];
    const float* __restrict__ c = cext ? cext : X + (int64_t)chosen[it - 1] * d;
    for (int j = threadIdx.x; j < d; j += KPP_THREADS) cs[j] = c[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double* sqb = sqs[w];
    float* tr = trs[w];
    double best = 0.0;
    for (int64_t row0 = (int64_t)blockIdx.x * KPP_THREADS; row0 < N; row0 += (int64_t)gridDim.x * KPP_THREADS) {
        const int64_t wr0 = row0 + 64 * w;             // this wave's rows wr0 .. wr0 + 63 (past N: row N - 1, dropped)
        const int64_t n = wr0 + lane;
        // this lane's 4 pieces: rows wr0 + q / 4 (q = 64 k + lane), dims 4 (q % 4) of each 16-dim step
        const int64_t r0 = wr0 + (lane >> 2), rlast = N - 1;
        const float* s0 = X + (r0 < N ? r0 : rlast) * d + 4 * (lane & 3);
        const float* s1 = X + (r0 + 16 < N ? r0 + 16 : rlast) * d + 4 * (lane & 3);
        const float* s2 = X + (r0 + 32 < N ? r0 + 32 : rlast) * d + 4 * (lane & 3);
        const float* s3 = X + (r0 + 48 < N ? r0 + 48 : rlast) * d + 4 * (lane & 3);
        float* t0 = tr + (lane >> 2) * KR_S + 4 * (lane & 3);
        float4 n0 = *reinterpret_cast<const float4*>(s0), n1 = *reinterpret_cast<const float4*>(s1);
        float4 n2 = *reinterpret_cast<const float4*>(s2), n3 = *reinterpret_cast<const float4*>(s3);
        double acc = 0.0;
        for (int j0 = 0; j0 < d; j0 += 16) {
            const float4 c0 = n0, c1 = n1, c2 = n2, c3 = n3;
            const int jn = j0 + 16 < d ? j0 + 16 : j0;     // the last step reloads its own (no branch)
            n0 = *reinterpret_cast<const float4*>(s0 + jn);
            n1 = *reinterpret_cast<const float4*>(s1 + jn);
            n2 = *reinterpret_cast<const float4*>(s2 + jn);
            n3 = *reinterpret_cast<const float4*>(s3 + jn);
            *reinterpret_cast<float4*>(t0) = c0;
            *reinterpret_cast<float4*>(t0 + 16 * KR_S) = c1;
            *reinterpret_cast<float4*>(t0 + 32 * KR_S) = c2;
            *reinterpret_cast<float4*>(t0 + 48 * KR_S) = c3;
            wave_sync();
            double df[16], p[16];
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const float4 v = *reinterpret_cast<const float4*>(tr + lane * KR_S + 4 * h);
                const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; u++) df[4 * h + u] = __dsub_rn((double)xv[u], (double)cs[j0 + 4 * h + u]);
            }
            wave_sync();
            gp_sq_wave<16, false>(df, p, sqb);
#pragma unroll
            for (int u = 0; u < 16; u++) acc = __dadd_rn(acc, p[u]);
        }
        const double m = n < N ? kpp_take_min(sqrt(acc), it, mind, n, best) : 0.0;
        kpp_group_sum(m * m, gsum, row0 / KPP_THREADS);
    }
    kpp_block_max(best, bmax);
}

// --------------------------------------------------------------------- (3)
// One block: the max of the minima (from the per-block maxima, written to
// mx_bits for the exact q_m), then the approximate chunk sums sum m^2 / max^2
// (two 256-row groups per chunk) and their exclusive scan (order irrelevant:
// guesses only).
constexpr int KPP_SCAN_THREADS = 1024;

// The block's fold of the per-block maxima (every thread gets it).
__device__ inline unsigned long long kpp_fold_max(const unsigned long long* __restrict__ bmax, int nb,
                                                  unsigned long long* redm) {
    unsigned long long mb = 0;
    for (int i = threadIdx.x; i < nb; i += KPP_SCAN_THREADS) mb = bmax[i] > mb ? bmax[i] : mb;
    redm[threadIdx.x] = mb;
    __syncthreads();
    for (int off = KPP_SCAN_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off && redm[threadIdx.x + off] > redm[threadIdx.x]) redm[threadIdx.x] = redm[threadIdx.x + off];
        __syncthreads();
    }
    return redm[0];
}

// Approximate chunk starts: start0 (the approximate sum before these rows; 0
// on one device) + the exclusive scan of the chunk sums sum m^2 / mx^2.
__device__ inline void kpp_chunk_starts(const double* __restrict__ gsum, int64_t ngroups, int64_t nch, double mx,
                                        double start0, double* __restrict__ chunk_start, double* part) {
    const double inv = 1.0 / (mx * mx);
    auto csum = [&](int64_t c) { return (gsum[2 * c] + (2 * c + 1 < ngroups ? gsum[2 * c + 1] : 0.0)) * inv; };
    const int64_t per = (nch + KPP_SCAN_THREADS - 1) / KPP_SCAN_THREADS;
    const int64_t lo = threadIdx.x * per, hi = lo + per < nch ? lo + per : nch;
    double v = 0.0;
    for (int64_t c = lo; c < hi; c++) v += csum(c);
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < KPP_SCAN_THREADS; off <<= 1) {   // inclusive scan of the partials
        const double o = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0.0;
        __syncthreads();
        part[threadIdx.x] += o;
        __syncthreads();
    }
    double run = start0 + (threadIdx.x ? part[threadIdx.x - 1] : 0.0);
    for (int64_t c = lo; c < hi; c++) {
        chunk_start[c] = run;
        run += csum(c);
    }
}

__global__ __launch_bounds__(KPP_SCAN_THREADS) void kpp_scan_kernel(
    const unsigned long long* __restrict__ bmax, int nb, const double* __restrict__ gsum, int64_t ngroups, int64_t nch,
    unsigned long long* __restrict__ mx_bits, double* __restrict__ chunk_start) {
    __shared__ unsigned long long redm[KPP_SCAN_THREADS];
    __shared__ double part[KPP_SCAN_THREADS];
    const unsigned long long mxb = kpp_fold_max(bmax, nb, redm);
    if (threadIdx.x == 0) *mx_bits = mxb;
    kpp_chunk_starts(gsum, ngroups, nch, __longlong_as_double((long long)mxb), 0.0, chunk_start, part);
}

// A shard's half of kpp_scan_kernel before the exchange: its own max and its
// sum m^2 (any order: guesses only), for the host.
__global__ __launch_bounds__(KPP_SCAN_THREADS) void kpp_fold_kernel(
    const unsigned long long* __restrict__ bmax, int nb, const double* __restrict__ gsum, int64_t ngroups,
    KppShardOut* __restrict__ out) {
    __shared__ unsigned long long redm[KPP_SCAN_THREADS];
    __shared__ double part[KPP_SCAN_THREADS];
    const unsigned long long mxb = kpp_fold_max(bmax, nb, redm);
    double v = 0.0;
    for (int64_t g = threadIdx.x; g < ngroups; g += KPP_SCAN_THREADS) v += gsum[g];
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = KPP_SCAN_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out->max_bits = mxb;
        out->sum = part[0];
    }
}

// ... and after it: the GLOBAL max (mx_bits, for the exact q_m) and the chunk
// starts from the approximate sum of the rows before this shard.
__global__ __launch_bounds__(KPP_SCAN_THREADS) void kpp_starts_kernel(
    const double* __restrict__ gsum, int64_t ngroups, int64_t nch, unsigned long long gmax_bits, double start0,
    unsigned long long* __restrict__ mx_bits, double* __restrict__ chunk_start) {
    __shared__ double part[KPP_SCAN_THREADS];
    if (threadIdx.x == 0) *mx_bits = gmax_bits;
    kpp_chunk_starts(gsum, ngroups, nch, __longlong_as_double((long long)gmax_bits), start0, chunk_start, part);
}

// Chunk guesses: each chunk's record (kpp_chunk_record) from its rows' units in
// the binade of its approximate start. A chunk with prefix arrays (a predicted
// crossing, a tie) gets them in binades e and e + 1 (pa, pb), so the walk
// resolves it with one hardware add per crossing or tie row instead of element
// by element. Thread t owns rows 2t, 2t+1 (row order for the scans).
__global__ __launch_bounds__(KPP_THREADS) void kpp_chunk_units_kernel(
    const double* __restrict__ mind, int64_t N, const unsigned long long* __restrict__ mx_bits, double* __restrict__ qbuf,
    const double* __restrict__ chunk_start, int64_t nch, KppChunk* __restrict__ meta, int64_t* __restrict__ pa,
    int64_t* __restrict__ pb) {
    static_assert(KPP_CHUNK == 2 * KPP_THREADS, "two rows per thread");
    __shared__ long long red[KPP_THREADS / 64];
    __shared__ int redc[KPP_THREADS / 64];
    __shared__ long long wtot[4][KPP_THREADS / 64];
    const int64_t c0 = (int64_t)blockIdx.x * KPP_CHUNK;
    const double a = chunk_start[blockIdx.x];
    // a guess only; tiny or non-finite starts are left to the exact walk
    const int e = kpp_binade0(a);
    const int64_t i0 = c0 + 2 * threadIdx.x;
    // q_m = (min_m / max)^2 (:121-124), stored for the walk
    const double mx = __longlong_as_double((long long)*mx_bits);
    const double q0 = i0 < N ? kpp_q(mind[i0], mx) : 0.0, q1 = i0 + 1 < N ? kpp_q(mind[i0 + 1], mx) : 0.0;
    if (i0 < N) qbuf[i0] = q0;
    if (i0 + 1 < N) qbuf[i0 + 1] = q1;
    int ca0, ca1;
    const int64_t ra0 = kpp_units(q0, e, ca0), ra1 = kpp_units(q1, e, ca1);
    long long v = ra0 + ra1;
    int cl = ca0 | ca1;
    for (int off = 32; off >= 1; off >>= 1) {
        v += __shfl_xor(v, off);
        cl |= __shfl_xor(cl, off);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[w] = v; redc[w] = cl; }
    __syncthreads();
    long long t = 0;
    int any = 0;
    for (int k = 0; k < KPP_THREADS / 64; k++) { t += red[k]; any |= redc[k]; }
    const bool has_next = blockIdx.x + 1 < nch;
    const KppChunk m = kpp_chunk_record(a, has_next, has_next ? chunk_start[blockIdx.x + 1] : 0.0, t, any);
    if (m.dual != 0) {                             // prefix arrays; block-uniform
        int cb0, cb1;
        const int64_t rb0 = kpp_units(q0, e + 1, cb0), rb1 = kpp_units(q1, e + 1, cb1);
        // values and unresolvable-row counts, scanned in row order
        int64_t sa = wave_incl_scan64(ra0 + ra1, lane), sb = wave_incl_scan64(rb0 + rb1, lane);
        int64_t sfa = wave_incl_scan64((ca0 == 2) + (ca1 == 2), lane), sfb = wave_incl_scan64((cb0 == 2) + (cb1 == 2), lane);
        if (lane == 63) { wtot[0][w] = sa; wtot[1][w] = sb; wtot[2][w] = sfa; wtot[3][w] = sfb; }
        __syncthreads();
        for (int k = 0; k < w; k++) { sa += wtot[0][k]; sb += wtot[1][k]; sfa += wtot[2][k]; sfb += wtot[3][k]; }
        // inclusive prefixes at rows 2t and 2t + 1
        if (i0 < N) {
            pa[i0] = kpp_entry(sa - ra1, sfa - (ca1 == 2), ca0);
            pb[i0] = kpp_entry(sb - rb1, sfb - (cb1 == 2), cb0);
        }
        if (i0 + 1 < N) {
            pa[i0 + 1] = kpp_entry(sa, sfa, ca1);
            pb[i0 + 1] = kpp_entry(sb, sfb, cb1);
        }
    }
    if (threadIdx.x == 0) meta[blockIdx.x] = m;
}

// The exact walk (one wave: kpp_walk, after its parts). s is uniform across the
// wave. A step covers 64 lanes x KPP_CPL consecutive chunks (lane-local prefix,
// then a wave scan of the lane totals); R < 2^53 per chunk keeps every prefix
// below 2^62. Starts from s (0 on one device and on the shard of global row 0,
// else the sum after the earlier shards' rows: a chunk's result depends on the rows
// before it through s alone), returns s after row N - 1; nseq counts the stop chunks.
constexpr int KPP_CPL = 8;                         // chunks per lane per step
constexpr int KPP_STEP = 64 * KPP_CPL;
constexpr int KPP_WIN = 2 * KPP_STEP;              // chunk records staged in LDS (16 KB)
constexpr int KPP_EPL = KPP_CHUNK / 64;            // rows of a chunk per lane
struct KppWalkLds {
    KppChunk wm[KPP_WIN];                          // the records of chunks win0 .. win0 + WIN - 1
    double qs[KPP_CHUNK];                          // a stop chunk's q and prefix arrays
    int64_t pas[KPP_CHUNK], pbs[KPP_CHUNK];
};

// (Re)fill the window at win0: all loads in flight before the LDS writes
// (clamped indices: a guarded load per element compiled to one round trip each).
__device__ __forceinline__ void kpp_fill(KppWalkLds& L, const KppChunk* __restrict__ meta, int64_t nch, int64_t win0,
                                         int lane) {
    KppChunk tmp[KPP_WIN / 64];
#pragma unroll
    for (int t = 0; t < KPP_WIN / 64; t++) {
        const int64_t j = win0 + lane + 64 * t;
        tmp[t] = meta[j < nch ? j : nch - 1];
    }
#pragma unroll
    for (int t = 0; t < KPP_WIN / 64; t++) L.wm[lane + 64 * t] = tmp[t];
    wave_sync();
}

// The integer step over chunks base .. base + STEP - 1 (inside the window):
// those before the first whose guess does not hold (kpp_guess_holds for the s
// it would start from) get their exact start in chunk_s and mode 0, and s moves
// past them. Returns that stop chunk (nch: the end), or -1 if all were resolved.
__device__ __forceinline__ int64_t kpp_step(const KppWalkLds& L, int64_t base, int64_t win0, int64_t nch,
                                            double* chunk_s, int32_t* chunk_mode, double& s, int lane) {
    const bool s_ok = kpp_usable(s);
    const int es = kpp_binade0(s);
    const int64_t s_units = s_ok ? kpp_to_units(s, es) : 0;
    const int64_t j0 = base + (int64_t)lane * KPP_CPL;
    int64_t R[KPP_CPL];
    int lbad = KPP_CPL;                            // first chunk of the lane with a wrong guess
    int64_t tot = 0;
#pragma unroll
    for (int t = 0; t < KPP_CPL; t++) {
        const int64_t j = j0 + t;
        KppChunk m;
        m.R = 0; m.e = KPP_DIRTY;
        if (j < nch) m = L.wm[j - win0];
        R[t] = m.R;
        tot += m.R;
        if (lbad == KPP_CPL && !(j < nch && kpp_guess_binade(s_ok, es, m))) lbad = t;
    }
    // exclusive prefix of the lane totals
    int64_t pre = wave_incl_scan64(tot, lane) - tot;
    // the lane's first chunk that is wrong or would leave the binade
    int first = lbad;
    int64_t run = s_units + pre;
#pragma unroll
    for (int t = 0; t < KPP_CPL; t++) {
        if (t < first && !kpp_fits(run, R[t])) first = t;
        if (t < first) run += R[t];
    }
    const unsigned long long bad = __ballot(first < KPP_CPL);
    const int fl = bad ? __ffsll((long long)bad) - 1 : 64;       // first lane with a stop
    // lanes before fl: all KPP_CPL chunks resolved; lane fl: its chunks before
    // `first` (lanes before fl have first == KPP_CPL)
    if (lane <= fl) {
        int64_t r = s_units + pre;
#pragma unroll
        for (int t = 0; t < KPP_CPL; t++) {
            if (t < first) {
                chunk_s[j0 + t] = kpp_from_units(r, es);
                chunk_mode[j0 + t] = 0;
                r += R[t];
            }
        }
    }
    const int fstop = fl < 64 ? __builtin_amdgcn_readlane(first, fl) : KPP_CPL;
    const int64_t c = base + (int64_t)(fl < 64 ? fl : 64) * KPP_CPL + (fl < 64 ? fstop : 0);
    // s after the resolved chunks: `run` of lane fl (or of lane 63 if none stopped)
    const int64_t adv = readlane64(run, fl < 64 ? fl : 63);
    if (c > base) s = kpp_from_units(adv, es);
    return fl == 64 ? -1 : c;
}

// Stage a stop chunk of n rows (q, pa, pb: at its first row): lane l holds rows
// 8l..8l+7 of the prefix arrays in registers; q and the arrays also go to LDS for
// the uniform reads; every load is issued before the first use (clamped indices).
__device__ __forceinline__ void kpp_stage(KppWalkLds& L, const double* __restrict__ q, const int64_t* __restrict__ pa,
                                          const int64_t* __restrict__ pb, int n, bool arrays, int64_t (&PA)[KPP_EPL],
                                          int64_t (&PB)[KPP_EPL], int lane) {
    double qv[KPP_EPL];
#pragma unroll
    for (int t = 0; t < KPP_EPL; t++) {
        const int i = lane * KPP_EPL + t;
        qv[t] = q[i < n ? i : n - 1];
    }
    if (arrays) {
#pragma unroll
        for (int t = 0; t < KPP_EPL; t++) {
            const int i = lane * KPP_EPL + t;
            PA[t] = pa[i < n ? i : n - 1];
            PB[t] = pb[i < n ? i : n - 1];
        }
    }
#pragma unroll
    for (int t = 0; t < KPP_EPL; t++) L.qs[lane * KPP_EPL + t] = qv[t];
    if (arrays) {
#pragma unroll
        for (int t = 0; t < KPP_EPL; t++) { L.pas[lane * KPP_EPL + t] = PA[t]; L.pbs[lane * KPP_EPL + t] = PB[t]; }
    }
    wave_sync();
}

// Rows [i0, m) of the staged chunk as integers in binade E from the prefix array
// P (in LDS; PR: this lane's entries; s exact, in binade E): returns m, the first
// row that stops (kpp_entry_stops); s moves to row m - 1. cum: at the chunk's row 0.
__device__ __forceinline__ int kpp_resolve(const int64_t* P, const int64_t (&PR)[KPP_EPL], int i0, int n, int E,
                                           double* cum, double& s, int lane) {
    const int64_t su = kpp_to_units(s, E);
    const int64_t base_p = i0 > 0 ? kpp_entry_prefix(P[i0 - 1]) : 0;
    int lf = KPP_EPL;
#pragma unroll
    for (int t = 0; t < KPP_EPL; t++) {
        const int i = lane * KPP_EPL + t;
        if (lf == KPP_EPL && i >= i0 && i < n && kpp_entry_stops(PR[t], su, base_p)) lf = t;
    }
    const unsigned long long fbits = __ballot(lf < KPP_EPL);
    const int fl = fbits ? __ffsll((long long)fbits) - 1 : 64;
    const int m = fl < 64 ? fl * KPP_EPL + __builtin_amdgcn_readlane(lf, fl) : n;
    double out[KPP_EPL];
#pragma unroll
    for (int t = 0; t < KPP_EPL; t++) out[t] = kpp_from_units(su + (kpp_entry_prefix(PR[t]) - base_p), E);
#pragma unroll
    for (int t = 0; t < KPP_EPL; t++) {
        const int i = lane * KPP_EPL + t;
        if (i >= i0 && i < m) cum[i] = out[t];
    }
    if (m > i0) s = kpp_from_units(su + (kpp_entry_prefix(P[m - 1]) - base_p), E);
    return m;
}

// The staged chunk through its prefix arrays in binades eg and eg + 1: the rows
// before a crossing from pa, the crossing (or tie) row by the reference's hardware
// add, the rows after it from pb. Returns the first row left to the tail (n: none).
__device__ __forceinline__ int kpp_two_binades(const KppWalkLds& L, const int64_t (&PA)[KPP_EPL],
                                               const int64_t (&PB)[KPP_EPL], int eg, int n, double* cum, double& s,
                                               int lane) {
    int i0 = 0;
    while (i0 < n) {
        if (!kpp_usable(s)) break;
        const int E = kpp_binade(s);
        if (E != eg && E != eg + 1) break;
        const int64_t* P = E == eg ? L.pas : L.pbs;
        i0 = E == eg ? kpp_resolve(L.pas, PA, i0, n, E, cum, s, lane) : kpp_resolve(L.pbs, PB, i0, n, E, cum, s, lane);
        if (i0 >= n || kpp_entry_poison(P[i0])) break;   // done, or an unresolvable row: one by one from it
        s = __dadd_rn(L.qs[i0], s);             // a tie or crossing row: the reference's add
        if (lane == 0) cum[i0] = s;
        i0++;
    }
    return i0;
}

// Rows i0 .. n - 1 one by one, the reference's adds (:122-125): every lane adds
// and stores the same value (one line, no exec toggling, ~26 cycles per row),
// the next 16 values read ahead from LDS with uniform-address (broadcast) reads.
__device__ __forceinline__ void kpp_tail(const double* qs, int i0, int n, double* cum, double& s) {
    constexpr int QB = 16;
    double qn[QB];
#pragma unroll
    for (int t = 0; t < QB; t++) qn[t] = qs[i0 + t < n ? i0 + t : n - 1];
    int i = i0;
    for (; i + QB <= n; i += QB) {
        double qv[QB];
#pragma unroll
        for (int t = 0; t < QB; t++) qv[t] = qn[t];
        if (i + 2 * QB <= n) {
#pragma unroll
            for (int t = 0; t < QB; t++) qn[t] = qs[i + QB + t];
        }
#pragma unroll
        for (int t = 0; t < QB; t++) {
            s = __dadd_rn(qv[t], s);           // the reference's add (0 + q_0 = q_0 for row 0)
            cum[i + t] = s;
        }
    }
    for (; i < n; i++) {
        s = __dadd_rn(qs[i], s);
        cum[i] = s;
    }
}

__device__ __forceinline__ double kpp_walk(
    const double* __restrict__ qbuf, int64_t N, const KppChunk* __restrict__ meta, int64_t nch,
    const int64_t* __restrict__ pa, const int64_t* __restrict__ pb, double* chunk_s, int32_t* chunk_mode, double* cum,
    double s, unsigned long long& nseq) {
    __shared__ KppWalkLds L;
    const int lane = threadIdx.x;
    int64_t base = 0, win0 = -2 * KPP_WIN;
    while (base < nch) {
        if (base < win0 || base + KPP_STEP > win0 + KPP_WIN) kpp_fill(L, meta, nch, win0 = base, lane);
        // now win0 <= base and base + STEP <= win0 + WIN: a stop chunk lies in the window
        const int64_t c = kpp_step(L, base, win0, nch, chunk_s, chunk_mode, s, lane);
        if (c < 0) {
            base += KPP_STEP;
            continue;
        }
        if (c >= nch) break;
        // Stop chunk c (the first, a binade crossing, a tie, a non-finite value):
        // through its prefix arrays if it has them, any rest (no arrays, a row
        // unresolvable in either binade, a third binade) row by row.
        const int64_t r0 = c * KPP_CHUNK;
        const int n = (int)(N - r0 < KPP_CHUNK ? N - r0 : KPP_CHUNK);
        if (lane == 0) {
            chunk_s[c] = s;
            chunk_mode[c] = 1;
        }
        const KppChunk mc = L.wm[c - win0];
        const bool arrays = mc.dual != 0;
        int64_t PA[KPP_EPL], PB[KPP_EPL];
        kpp_stage(L, qbuf + r0, pa + r0, pb + r0, n, arrays, PA, PB, lane);
        const int i0 = arrays ? kpp_two_binades(L, PA, PB, mc.dual - 2048, n, cum + r0, s, lane) : 0;
        kpp_tail(L.qs, i0, n, cum + r0, s);
        wave_sync();
        base = c + 1;
        nseq++;
    }
    return s;
}

// The reference's binary search (:132-149) = the first row whose prefix sum
// reaches rd, for rd <= total (the sum after row N - 1; the sums never
// decrease). The prefix sums are never materialised: the chunk by a 64-ary
// search over the chunk ends, then its rows (the walk wrote a stop chunk's; an
// integer chunk's are formed here). One wave, after kpp_walk.
__device__ __forceinline__ int64_t kpp_search(const double* __restrict__ qbuf, int64_t N,
                                              const KppChunk* __restrict__ meta, int64_t nch, const double* chunk_s,
                                              const int32_t* chunk_mode, const double* cum, double total, double rd) {
    const int lane = threadIdx.x;
    auto chunk_end = [&](int64_t cc) -> double { return cc + 1 < nch ? chunk_s[cc + 1] : total; };
    int64_t lo = 0, hi = nch;              // the first chunk whose end reaches rd lies in [lo, hi)
    while (hi - lo > 64) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t p = lo + (int64_t)(lane + 1) * step - 1;
        const bool ge = p >= hi - 1 || chunk_end(p) >= rd;
        const unsigned long long b = __ballot(ge);
        const int f = __ffsll((long long)b) - 1;          // lane 63 always qualifies
        const int64_t nlo = f > 0 ? lo + (int64_t)f * step : lo;
        const int64_t nhi = lo + (int64_t)(f + 1) * step;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    const bool ge = lo + lane >= hi - 1 || chunk_end(lo + lane) >= rd;
    const int64_t cs_ = lo + (__ffsll((long long)__ballot(ge)) - 1);
    // rows of chunk cs_
    const int64_t r0 = cs_ * KPP_CHUNK;
    const int n = (int)(N - r0 < KPP_CHUNK ? N - r0 : KPP_CHUNK);
    double v[KPP_EPL];
    if (chunk_mode[cs_] != 0) {
#pragma unroll
        for (int t = 0; t < KPP_EPL; t++) {
            const int i = lane * KPP_EPL + t;
            v[t] = cum[r0 + (i < n ? i : n - 1)];
        }
    } else {
        const int e = meta[cs_].e;          // a mode-0 chunk is clean: every row of class 0
        const int64_t su = kpp_to_units(chunk_s[cs_], e);
        int64_t r[KPP_EPL], own = 0;
#pragma unroll
        for (int t = 0; t < KPP_EPL; t++) {
            const int i = lane * KPP_EPL + t;
            int cls;
            r[t] = i < n ? kpp_units(qbuf[r0 + i], e, cls) : 0;
            own += r[t];
        }
        int64_t run = su + wave_incl_scan64(own, lane) - own;
#pragma unroll
        for (int t = 0; t < KPP_EPL; t++) {
            run += r[t];
            v[t] = kpp_from_units(run, e);
        }
    }
    int lf = KPP_EPL;
#pragma unroll
    for (int t = 0; t < KPP_EPL; t++)
        if (lf == KPP_EPL && lane * KPP_EPL + t < n && v[t] >= rd) lf = t;
    const unsigned long long b = __ballot(lf < KPP_EPL);
    const int fl = b ? __ffsll((long long)b) - 1 : 63;      // b != 0: the chunk's end reaches rd
    return r0 + fl * KPP_EPL + __builtin_amdgcn_readlane(lf, fl);
}

__device__ inline void kpp_walk_stats(unsigned long long* __restrict__ stats, int64_t nch, unsigned long long nseq) {
    if (threadIdx.x == 0 && stats) {
        atomicAdd(stats + STAT_KPP_CHUNKS, (unsigned long long)nch);
        atomicAdd(stats + STAT_KPP_SEQ, nseq);
    }
}

// One device: the walk from 0, then (4) the draw (:127-149): rd =
// uniform_real(0, total) = canon * (total - 0) + 0 and the search (rd <=
// total; a NaN total from degenerate minima gives rd NaN and row 0).
__global__ __launch_bounds__(64) void kpp_chain_kernel(
    const double* __restrict__ qbuf, int64_t N, const KppChunk* __restrict__ meta, int64_t nch,
    const int64_t* __restrict__ pa, const int64_t* __restrict__ pb, double* chunk_s, int32_t* chunk_mode, double* cum,
    const double* __restrict__ canon, int it, int32_t* __restrict__ chosen, unsigned long long* __restrict__ stats) {
    unsigned long long nseq = 0;
    const double total = kpp_walk(qbuf, N, meta, nch, pa, pb, chunk_s, chunk_mode, cum, 0.0, nseq);
    __threadfence();                               // this wave's chunk_s / cum stores, visible to its loads
    const double rd = __dadd_rn(__dmul_rn(canon[it], __dsub_rn(total, 0.0)), 0.0);
    int64_t pick = 0;
    if (rd > qbuf[0])                              // cum[0] = 0 + q_0 = q_0
        pick = kpp_search(qbuf, N, meta, nch, chunk_s, chunk_mode, cum, total, rd);
    if (threadIdx.x == 0) chosen[it] = (int32_t)pick;
    kpp_walk_stats(stats, nch, nseq);
}

// A shard's walk: from s_in (the sum after the earlier shards' rows; with
// s_in > 0 its first chunk has a binade and takes the integer path like any
// other) to s_out; the draw waits for the last shard's s_out, the total.
__global__ __launch_bounds__(64) void kpp_chain_shard_kernel(
    const double* __restrict__ qbuf, int64_t N, const KppChunk* __restrict__ meta, int64_t nch,
    const int64_t* __restrict__ pa, const int64_t* __restrict__ pb, double* chunk_s, int32_t* chunk_mode, double* cum,
    double s_in, KppShardOut* __restrict__ out, unsigned long long* __restrict__ stats) {
    unsigned long long nseq = 0;
    const double s = kpp_walk(qbuf, N, meta, nch, pa, pb, chunk_s, chunk_mode, cum, s_in, nseq);
    if (threadIdx.x == 0) out->s_out = s;
    kpp_walk_stats(stats, nch, nseq);
}

// A shard's part of the search for the draw rd (formed on the host from the
// total): its first row whose prefix sum reaches rd, or -1. The shard of
// global row 0 answers row 0 unless rd > q_0 (:139; a NaN rd as well).
__global__ __launch_bounds__(64) void kpp_pick_shard_kernel(
    const double* __restrict__ qbuf, int64_t N, const KppChunk* __restrict__ meta, int64_t nch, const double* chunk_s,
    const int32_t* chunk_mode, const double* cum, double rd, int owns_row0, KppShardOut* out) {
    const double total = out->s_out;
    int64_t pick = -1;
    if (owns_row0 && !(rd > qbuf[0])) pick = 0;
    else if (total >= rd) pick = kpp_search(qbuf, N, meta, nch, chunk_s, chunk_mode, cum, total, rd);
    if (threadIdx.x == 0) out->pick = pick;
}

// The workspace's regions as pointers (kpp_layout.h: the map).
struct KppWs {
    int64_t nch, ngroups;
    unsigned dgrid;
    double *mind, *cum, *gsum, *cstart, *cs, *qbuf;
    KppChunk* meta;
    int32_t* mode;
    unsigned long long *mx, *bmax;
    KppShardOut* out;
    int64_t *pa, *pb;
};
static KppWs kpp_carve(void* ws, int64_t N) {
    const KppLayout l = kpp_layout(N);
    char* p = (char*)ws;
    KppWs w;
    w.nch = l.nch; w.ngroups = l.ngroups; w.dgrid = l.dgrid;
    w.mind = (double*)(p + l.mind);      w.cum = (double*)(p + l.cum);
    w.gsum = (double*)(p + l.gsum);      w.cstart = (double*)(p + l.cstart);
    w.meta = (KppChunk*)(p + l.meta);    w.cs = (double*)(p + l.cs);
    w.mode = (int32_t*)(p + l.mode);     w.mx = (unsigned long long*)(p + l.mx);
    w.out = (KppShardOut*)(p + l.out);   w.bmax = (unsigned long long*)(p + l.bmax);
    w.qbuf = (double*)(p + l.qbuf);      w.pa = (int64_t*)(p + l.pa);
    w.pb = (int64_t*)(p + l.pb);
    return w;
}

// The distance pass of iteration `it` against the newest centroid: row
// chosen[it - 1] of X, or the [d] row cext of X's type (a shard: the row
// usually lies on another rank).
static void kpp_launch_dist(hipStream_t s, Pts X, int64_t N, int d, int metric, const int32_t* chosen, const void* cext,
                            int it, const KppWs& w) {
    const bool vec = d % KPP_DJ == 0 && !X.f64;
    const auto go = [&](auto kernel, const auto* x) {          // dynamic LDS: the centroid row
        hipLaunchKernelGGL(kernel, dim3(w.dgrid), dim3(KPP_THREADS), sizeof(*x) * d, s, x, N, d, chosen, (decltype(x))cext, it,
                           w.mind, w.bmax, w.gsum);
    };
    if (X.f64) metric == 0 ? go(kpp_dist_kernel<0, false, double>, X.d()) : go(kpp_dist_kernel<1, false, double>, X.d());
    else if (metric == 0) vec ? go(kpp_dist_reg_kernel, X.f()) : go(kpp_dist_kernel<0, false, float>, X.f());
    else vec ? go(kpp_dist_kernel<1, true, float>, X.f()) : go(kpp_dist_kernel<1, false, float>, X.f());
}

// Runs iterations 1..K-1; chosen[0] and canon[1..K-1] are already on the device.
int launch_kmeans_pp(hipStream_t s, Pts X, int64_t N, int d, int K, int metric, const double* canon,
                     int32_t* chosen, void* ws, unsigned long long* stats) {
    const KppWs w = kpp_carve(ws, N);
    for (int it = 1; it < K; it++) {
        kpp_launch_dist(s, X, N, d, metric, chosen, nullptr, it, w);
        hipLaunchKernelGGL(kpp_scan_kernel, dim3(1), dim3(KPP_SCAN_THREADS), 0, s, w.bmax, (int)w.dgrid, w.gsum, w.ngroups, w.nch,
                           w.mx, w.cstart);
        hipLaunchKernelGGL(kpp_chunk_units_kernel, dim3((unsigned)w.nch), dim3(KPP_THREADS), 0, s, w.mind, N, w.mx, w.qbuf,
                           w.cstart, w.nch, w.meta, w.pa, w.pb);
        hipLaunchKernelGGL(kpp_chain_kernel, dim3(1), dim3(64), 0, s, w.qbuf, N, w.meta, w.nch, w.pa, w.pb, w.cs, w.mode, w.cum,
                           canon, it, chosen, stats);
        if (const int rc = kstatus("kmeanspp.hip")) return rc;
    }
    return 0;
}

// ------------------------------------------------------------- row shards
// One iteration over contiguous row shards (lshkm_kpp_shard_*): the same
// kernels per shard, the same workspace (n >= 1 rows; the callers skip an empty
// shard), with the host between the steps: dist -> (max, sum m^2) of the shard;
// units with the global max and the approximate sum before the shard; chain
// from the exact s after the previous shard; pick for the draw. Each step's
// host-read values lie in the workspace's KppShardOut (kpp_layout(n).out).
int launch_kpp_shard_dist(hipStream_t s, Pts X, int64_t n, int d, int metric, const void* crow, int it, void* ws) {
    const KppWs w = kpp_carve(ws, n);
    kpp_launch_dist(s, X, n, d, metric, nullptr, crow, it, w);
    hipLaunchKernelGGL(kpp_fold_kernel, dim3(1), dim3(KPP_SCAN_THREADS), 0, s, w.bmax, (int)w.dgrid, w.gsum, w.ngroups, w.out);
    return kstatus("kmeanspp.hip (shard dist)");
}

int launch_kpp_shard_units(hipStream_t s, int64_t n, unsigned long long gmax_bits, double start, void* ws) {
    const KppWs w = kpp_carve(ws, n);
    hipLaunchKernelGGL(kpp_starts_kernel, dim3(1), dim3(KPP_SCAN_THREADS), 0, s, w.gsum, w.ngroups, w.nch, gmax_bits, start,
                       w.mx, w.cstart);
    hipLaunchKernelGGL(kpp_chunk_units_kernel, dim3((unsigned)w.nch), dim3(KPP_THREADS), 0, s, w.mind, n, w.mx, w.qbuf, w.cstart,
                       w.nch, w.meta, w.pa, w.pb);
    return kstatus("kmeanspp.hip (shard units)");
}

int launch_kpp_shard_chain(hipStream_t s, int64_t n, double s_in, void* ws, unsigned long long* stats) {
    const KppWs w = kpp_carve(ws, n);
    hipLaunchKernelGGL(kpp_chain_shard_kernel, dim3(1), dim3(64), 0, s, w.qbuf, n, w.meta, w.nch, w.pa, w.pb, w.cs, w.mode, w.cum,
                       s_in, w.out, stats);
    return kstatus("kmeanspp.hip (shard chain)");
}

int launch_kpp_shard_pick(hipStream_t s, int64_t n, double rd, int owns_row0, void* ws) {
    const KppWs w = kpp_carve(ws, n);
    hipLaunchKernelGGL(kpp_pick_shard_kernel, dim3(1), dim3(64), 0, s, w.qbuf, n, w.meta, w.nch, w.cs, w.mode, w.cum, rd,
                       owns_row0, w.out);
    return kstatus("kmeanspp.hip (shard pick)");
}

}  // namespace lshkm
