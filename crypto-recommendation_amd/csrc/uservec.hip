// uservec.hip — user vectors from scored tweets, exact, on gfx950.
//
//   tweets_to_user_vectors     lib/crypto_rec.hpp:78-140
//   clusters_to_user_vectors   lib/crypto_rec.hpp:143-210
//
// Both reduce to one primitive over a list of visits (tweet, group) in the
// reference's loop order: v[g][j] = v[g][j] + score for every
// coin j of the tweet when score > 0, known[g][j] = 1 either way. Each v[g][j]
// is a sequential fp64 chain, so the order is the result:
//
//   uv_count / scan / uv_expand: the visits become (key = g * C + j, tweet)
//     incidences in visit order (score > 0 only; the flags are set for all);
//   stable sort by key (scatter.hip) + csr_bounds: chain k's terms, in visit
//     order, are vals[row_ptr[k] .. row_ptr[k+1]);
//   uv_chain_short: one lane per chain of fewer than UV_LONG terms, real adds;
//   uv_chain_long: one wave per longer chain, 64 terms per step.
//
// The long chain's step. Every term is positive, so the running sum s never
// decreases. While s = S u stays in one binade (u its unit in the last place,
// 2^52 <= S < 2^53), adding x gives S + RN(x / u) exactly, provided x / u is no
// half-integer (a tie would round by the parity of S) and the result stays
// below 2^53 units. The prefixes are monotone, so the last one bounds them all:
// a batch of 64 is the integer sum of the RN(x / u) when none is a tie and
// S + sum <= 2^53 - 1; otherwise the batch is added term by term with hardware
// adds. This is kmseg.h's argument (ks_step_m's shifter) without the lower
// bound, which positive terms cannot cross.
//
// uv_fin_*: the finishing loop (:107-137, :177-207), one lane per group, the
// known sum sequential in i; the kept groups are compacted in group order by
// two scans.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "uvchain.h"

namespace lshkm {

constexpr int UV_THREADS = 256;

// bit 0: a tw outside [-1, T); 1: a grp outside [-1, G); 2: a ci_idx outside [0, C); 3: ci_ptr decreases or starts below 0
__global__ __launch_bounds__(UV_THREADS) void uv_check_visits(UvVisits q, uint32_t* __restrict__ flag) {
    const int64_t n = max(q.V, q.T);
    uint32_t f = 0;
    for (int64_t i = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * UV_THREADS) {
        if (i < q.V) {
            const int64_t tw = q.tw[i], g = q.grp[i];
            if (tw < -1 || tw >= q.T) f |= 1u;
            if (g < -1 || g >= q.G) f |= 2u;
        }
        if (i < q.T) {
            const int64_t a = q.ci_ptr[i], b = q.ci_ptr[i + 1];
            if (a < 0 || b < a || (i == 0 && a != 0)) f |= 8u;
        }
    }
    if (f) atomicOr(flag, f);
}

// after uv_check_visits passed: every [ci_ptr[t], ci_ptr[t+1]) is a range of ci_idx
__global__ __launch_bounds__(UV_THREADS) void uv_check_coins(UvVisits q, uint32_t* __restrict__ flag) {
    uint32_t f = 0;
    for (int64_t t = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x; t < q.T; t += (int64_t)gridDim.x * UV_THREADS) {
        const int64_t a = q.ci_ptr[t], b = q.ci_ptr[t + 1];
        for (int64_t p = a; p < b; p++) {
            const int32_t j = q.ci_idx[p];
            if (j < 0 || j >= q.C) f |= 4u;
        }
    }
    if (f) atomicOr(flag, f);
}

__device__ inline bool uv_live(const UvVisits& q, int64_t v, int64_t& tw, int64_t& g) {
    tw = q.tw[v];
    g = q.grp[v];
    return tw >= 0 && g >= 0;
}

// cnt[v] = the incidences visit v adds to chains: its tweet's coins when score > 0
__global__ __launch_bounds__(UV_THREADS) void uv_count(UvVisits q, int64_t* __restrict__ cnt) {
    for (int64_t v = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x; v < q.V; v += (int64_t)gridDim.x * UV_THREADS) {
        int64_t tw, g;
        const bool live = uv_live(q, v, tw, g);
        cnt[v] = live && q.score[tw] > 0 ? q.ci_ptr[tw + 1] - q.ci_ptr[tw] : 0;     // NaN > 0 is false
    }
}

__global__ __launch_bounds__(UV_THREADS) void uv_known_init(const uint8_t* __restrict__ carry, int64_t n,
                                                            uint8_t* __restrict__ known) {
    for (int64_t i = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * UV_THREADS)
        known[i] = carry ? (uint8_t)(carry[i] != 0) : (uint8_t)0;
}

// The flags (racing stores of the same byte) and the incidences, in visit order.
__global__ __launch_bounds__(UV_THREADS) void uv_expand(UvVisits q, const int64_t* __restrict__ off,
                                                        uint8_t* __restrict__ known, int32_t* __restrict__ keys,
                                                        int32_t* __restrict__ vals) {
    for (int64_t v = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x; v < q.V; v += (int64_t)gridDim.x * UV_THREADS) {
        int64_t tw, g;
        if (!uv_live(q, v, tw, g)) continue;
        const int64_t a = q.ci_ptr[tw], b = q.ci_ptr[tw + 1];
        const bool add = q.score[tw] > 0;
        int64_t o = off[v];
        for (int64_t p = a; p < b; p++) {
            const int64_t key = g * q.C + q.ci_idx[p];
            known[key] = 1;
            if (add) {
                keys[o] = (int32_t)key;
                vals[o] = (int32_t)tw;
                o++;
            }
        }
    }
}

constexpr int UV_LONG = 128;     // chains of this many terms or more: one wave each
constexpr int UV_BATCHES = 4;    // 64-term batches whose loads are in flight together

// One lane per chain; the chains of >= UV_LONG terms are listed for uv_chain_long.
__global__ __launch_bounds__(UV_THREADS) void uv_chain_short(const int64_t* __restrict__ row_ptr,
                                                             const int32_t* __restrict__ vals,
                                                             const double* __restrict__ score,
                                                             const double* __restrict__ carry, int64_t nkeys,
                                                             double* __restrict__ sum, int32_t* __restrict__ long_list,
                                                             uint32_t* __restrict__ long_count) {
    const int64_t k = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x;
    const bool in = k < nkeys;
    const int64_t a = in ? row_ptr[k] : 0, b = in ? row_ptr[k + 1] : 0;
    const bool is_long = b - a >= UV_LONG;
    seg_append(is_long, (int32_t)k, long_count, long_list, (int)(threadIdx.x & 63));
    if (!in || is_long) return;
    double s = carry ? carry[k] : 0.0;
    for (int64_t e = a; e < b; e++) s = __dadd_rn(s, score[vals[e]]);
    sum[k] = s;
}

__device__ inline uint64_t uv_wave_sum(uint64_t m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += (uint64_t)__shfl_xor((unsigned long long)m, o);
    return m;
}

// One batch of n <= 64 terms (lane l holds term l; 0.0 past n) onto the
// wave-uniform running sum s.
__device__ inline double uv_batch(double s, double x, int n) {
    const int be = uv_binade(s);
    if (be) {
        const KsStep t = uv_step(x, be);
        // every term summarised (no tie, none too large) and the last prefix inside the binade
        if (!__ballot(!t.ok) && uv_advance(s, be, uv_wave_sum((uint64_t)t.r))) return s;      // the sum < 64 * 2^51
    }
    for (int i = 0; i < n; i++) s = KS_ADD(s, __shfl(x, i));
    return s;
}

__global__ __launch_bounds__(UV_THREADS) void uv_chain_long(const int64_t* __restrict__ row_ptr,
                                                            const int32_t* __restrict__ vals,
                                                            const double* __restrict__ score,
                                                            const double* __restrict__ carry,
                                                            const int32_t* __restrict__ long_list,
                                                            const uint32_t* __restrict__ long_count,
                                                            double* __restrict__ sum) {
    const int lane = threadIdx.x & 63;
    const uint32_t nl = *long_count;
    const uint32_t nwaves = gridDim.x * (UV_THREADS / 64);
    for (uint32_t c = blockIdx.x * (UV_THREADS / 64) + (threadIdx.x >> 6); c < nl; c += nwaves) {
        const int64_t k = long_list[c];
        const int64_t a = row_ptr[k], b = row_ptr[k + 1];
        double s = carry ? carry[k] : 0.0;
        for (int64_t e0 = a; e0 < b; e0 += 64 * UV_BATCHES) {
            double x[UV_BATCHES];
#pragma unroll
            for (int u = 0; u < UV_BATCHES; u++) {
                const int64_t e = e0 + u * 64 + lane;
                x[u] = e < b ? score[vals[e]] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < UV_BATCHES; u++) {
                const int64_t left = b - (e0 + u * 64);                     // wave-uniform
                if (left > 0) s = uv_batch(s, x[u], (int)min(left, (int64_t)64));
            }
        }
        if (lane == 0) sum[k] = s;
    }
}

size_t uv_sort_bytes(int64_t E, int64_t nkeys) { return sort_scratch_bytes(E, nkeys); }

int launch_uv_check(hipStream_t s, const UvVisits& q, bool coins, uint32_t* flag) {
    if (coins)
        hipLaunchKernelGGL(uv_check_coins, dim3(gsz(q.T, UV_THREADS, 4096)), dim3(UV_THREADS), 0, s, q, flag);
    else
        hipLaunchKernelGGL(uv_check_visits, dim3(gsz(std::max(q.V, q.T), UV_THREADS, 4096)), dim3(UV_THREADS), 0, s, q,
                           flag);
    return kstatus("uservec.hip");
}

int launch_uv_count(hipStream_t s, const UvVisits& q, int64_t* cnt) {
    hipLaunchKernelGGL(uv_count, dim3(gsz(q.V, UV_THREADS, 8192)), dim3(UV_THREADS), 0, s, q, cnt);
    return kstatus("uservec.hip");
}

// The flags from the carry and the visits, the incidences sorted by key, and
// every chain. keys / vals / keys_s / vals_s: E int32 each; sort_ws:
// uv_sort_bytes(E, G * C); row_ptr: G * C + 1; long_list: G * C int32;
// long_count: one zeroed word.
int launch_uv_sums(hipStream_t s, const UvVisits& q, const int64_t* off, int64_t E, const double* carry_sum,
                   const uint8_t* carry_known, int32_t* keys, int32_t* vals, int32_t* keys_s, int32_t* vals_s,
                   void* sort_ws, int64_t* row_ptr, int32_t* long_list, uint32_t* long_count, double* sum,
                   uint8_t* known) {
    const int64_t nkeys = q.G * q.C;
    if (nkeys <= 0) return 0;
    hipLaunchKernelGGL(uv_known_init, dim3(gsz(nkeys, UV_THREADS, 4096)), dim3(UV_THREADS), 0, s, carry_known, nkeys,
                       known);
    if (q.V > 0)
        hipLaunchKernelGGL(uv_expand, dim3(gsz(q.V, UV_THREADS, 8192)), dim3(UV_THREADS), 0, s, q, off, known, keys, vals);
    int rc;
    if ((rc = kstatus("uservec.hip")) || (rc = stable_sort_by_key(s, keys, 1, vals, E, nkeys, keys_s, vals_s, sort_ws)) ||
        (rc = launch_csr_bounds(s, keys_s, E, nkeys, row_ptr)))
        return rc;
    hipLaunchKernelGGL(uv_chain_short, dim3((unsigned)((nkeys + UV_THREADS - 1) / UV_THREADS)), dim3(UV_THREADS), 0, s,
                       row_ptr, vals_s, q.score, carry_sum, nkeys, sum, long_list, long_count);
    // at most E / UV_LONG long chains; the waves stride over the list
    const int64_t max_long = std::min(E / UV_LONG, nkeys);
    if (max_long > 0)
        hipLaunchKernelGGL(uv_chain_long, dim3(gsz(max_long, UV_THREADS / 64, 2048)), dim3(UV_THREADS), 0, s, row_ptr,
                           vals_s, q.score, carry_sum, long_list, long_count, sum);
    return kstatus("uservec.hip");
}

// ------------------------------------------------------------------- finish
// crypto_rec.hpp:107-124 for group g: kept[g] (1: not useless), nunk[g] (the
// unknown set's size where kept, else 0), mean[g] = sum / known_number.
__global__ __launch_bounds__(UV_THREADS) void uv_fin_count(const double* __restrict__ sum,
                                                           const uint8_t* __restrict__ known, int64_t G, int C,
                                                           int64_t* __restrict__ kept, int64_t* __restrict__ nunk,
                                                           double* __restrict__ mean) {
    const int64_t g = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x;
    if (g >= G) return;
    double s = 0;
    int nk = 0, nu = 0;
    bool useless = true;
    for (int i = 0; i < C; i++) {
        const double v = sum[g * C + i];
        if (known[g * C + i] == 0) nu++;
        else { s = __dadd_rn(s, v); nk++; }
        if (v != 0) useless = false;
    }
    kept[g] = useless ? 0 : 1;
    nunk[g] = useless ? 0 : nu;
    mean[g] = __ddiv_rn(s, (double)nk);
}

__global__ __launch_bounds__(UV_THREADS) void uv_fin_write(const double* __restrict__ sum,
                                                           const uint8_t* __restrict__ known, int64_t G, int C,
                                                           const int64_t* __restrict__ row_off,
                                                           const int64_t* __restrict__ unk_off,
                                                           const double* __restrict__ mean, double* __restrict__ U,
                                                           double* __restrict__ mean_out, int64_t* __restrict__ unk_ptr,
                                                           int32_t* __restrict__ unk_idx, int32_t* __restrict__ src) {
    const int64_t g = (int64_t)blockIdx.x * UV_THREADS + threadIdx.x;
    if (g == 0) unk_ptr[row_off[G]] = unk_off[G];
    if (g >= G || row_off[g + 1] == row_off[g]) return;
    const int64_t r = row_off[g];
    const double m = mean[g];
    int64_t p = unk_off[g];
    mean_out[r] = m;
    src[r] = (int32_t)g;
    unk_ptr[r] = p;
    for (int i = 0; i < C; i++) {
        const bool kn = known[g * C + i] != 0;
        U[r * C + i] = kn ? sum[g * C + i] : m;
        if (!kn) unk_idx[p++] = i;
    }
}

// kept / nunk: G int64; row_off / unk_off: G + 1 int64; mean: G doubles; scan_ws: scan_ws_bytes(G)
int launch_uv_finish(hipStream_t s, const double* sum, const uint8_t* known, int64_t G, int C, int64_t* kept,
                     int64_t* nunk, int64_t* row_off, int64_t* unk_off, double* mean, int64_t* scan_ws, double* U,
                     double* mean_out, int64_t* unk_ptr, int32_t* unk_idx, int32_t* src) {
    const unsigned grid = (unsigned)((G + UV_THREADS - 1) / UV_THREADS);
    hipLaunchKernelGGL(uv_fin_count, dim3(grid), dim3(UV_THREADS), 0, s, sum, known, G, C, kept, nunk, mean);
    int rc;
    if ((rc = kstatus("uservec.hip")) || (rc = launch_scan_i64(s, kept, G, row_off, scan_ws)) ||
        (rc = launch_scan_i64(s, nunk, G, unk_off, scan_ws)))
        return rc;
    hipLaunchKernelGGL(uv_fin_write, dim3(grid), dim3(UV_THREADS), 0, s, sum, known, G, C, row_off, unk_off, mean, U,
                       mean_out, unk_ptr, unk_idx, src);
    return kstatus("uservec.hip");
}

}  // namespace lshkm
