// knn.hip — lshkm_knn: the k exact nearest rows of every
// query, ordered by (distance, key) with the NaN distances last.
//
// The screen is lshkm_min_vector_dist's (nearest.hip, §5f): the same blocks,
// LDS staging, MFMA chain, value v~ and radius E per (query, row) pair, over
// the same f32 images. What is done with the interval differs:
//   1. the rows are cut into disjoint groups; pass 1 writes the key of each
//      (query, group)'s smallest hi = v~ + E;
//   2. a select kernel takes the k-th smallest key of each query: tau. The k
//      smallest group minima are the hi of k distinct real rows, so the k-th
//      smallest exact distance is <= tau;
//   3. pass 2 keeps the rows with lo = v~ - E <= tau (capacity cap; a longer
//      list flags the query for the scan). A row that is not kept has an exact
//      distance > tau, above k kept rows': it is none of the k nearest.
// Both passes compute the same v~ and E, so the k rows that set tau are kept,
// and the kept set is a function of the inputs alone: tau is final before pass
// 2 starts, and the settle orders by (value, row), not by arrival.
//
// The settle: one wave per query over its kept rows and the call's poison
// rows, the exact chains of nearest_dev.h, 64 at a time, merged into a sorted
// list of 64 held one slot per lane. The same kernel serves the lists form
// (key = the position in the caller's list). The scan: one block per handed
// query over all N rows, a list per wave, joined at the end.
#include "../../include/lshkm.h"
#include "common.h"
#include "exact.h"
#include "kernels.h"
#include "knn_layout.h"
#include "nearest_dev.h"

#include <type_traits>

namespace lshkm {

static_assert(KNN_KMAX == 64, "a result slot per lane");
static_assert(KNN_GROUPS_MAX % 64 == 0, "the select wave holds a query's keys in whole registers");
constexpr uint32_t KNN_NO_KEY = 0xFFFFFFFFu;

// PASS 1: the (query, group) keys; PASS 2: the kept rows. The staging and the
// pair's v~ and E are nearest_screen_kernel's, instruction for instruction.
template <int DP, bool COS, int PASS>
__global__ __launch_bounds__(256, 2) void knn_screen_kernel(NearestSide rows, NearestSide qs, KnnKept kept) {
    constexpr int H = DP / 2;     // dims per lane half
    constexpr int DS = DP + 4;    // padded LDS row stride (floats): conflict-free ds_read_b128
    constexpr float C0 = COS ? nearest_e0_cos<DP>() : nearest_c1_euc<DP>();
    __shared__ __attribute__((aligned(16))) float cs[NEAREST_STAGE * DS];
    __shared__ float ra[NEAREST_STAGE], rrel[NEAREST_STAGE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int64_t uq = (int64_t)blockIdx.x * NEAREST_COLS + wave * 32 + col;    // this lane's query (both halves)
    const bool own = uq < qs.n;

    float b[H];
#pragma unroll
    for (int s = 0; s < H; s++) b[s] = own ? qs.xh[(size_t)uq * DP + h * H + s] : 0.f;
    const float qa = own ? qs.a[uq] : -1.f;
    const float qc = C0 + (own ? qs.rel[uq] : 0.f);
    bool alive = own && qa >= 0.f;
    uint32_t T = 0u;
    if (PASS == 2 && alive) {
        T = kept.tau[uq];
        alive = T != KNN_NO_KEY;             // fewer than k groups with a real row: the scan's
    }
    float mn = __builtin_inff();
    const int64_t r0 = (int64_t)blockIdx.y * kept.seg_rows, r1 = min(rows.n, r0 + kept.seg_rows);
    const int64_t grp_mask = ((int64_t)1 << kept.grp_shift) - 1;
    constexpr int PRE = NEAREST_STAGE * DP / 4 / 256;      // float4 per thread and step
    float4 pre[PRE];
    float pa = -1.f, prel = 0.f;
    auto fetch = [&](int64_t m0) {
#pragma unroll
        for (int i = 0; i < PRE; i++) {
            const int e4 = threadIdx.x + 256 * i, r = e4 / (DP / 4), j = (e4 % (DP / 4)) * 4;
            pre[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m0 + r < r1) pre[i] = *reinterpret_cast<const float4*>(rows.xh + (size_t)(m0 + r) * DP + j);
        }
        if (threadIdx.x < NEAREST_STAGE) {
            const int64_t m = m0 + threadIdx.x;
            pa = m < r1 ? rows.a[m] : -1.f;                  // negative: no row, or a poison one (the settle's)
            prel = m < r1 ? rows.rel[m] : 0.f;
        }
    };
    if (r0 < r1) fetch(r0);
    for (int64_t m0 = r0; m0 < r1; m0 += NEAREST_STAGE) {
#pragma unroll
        for (int i = 0; i < PRE; i++) {
            const int e4 = threadIdx.x + 256 * i, r = e4 / (DP / 4), j = (e4 % (DP / 4)) * 4;
            *reinterpret_cast<float4*>(cs + r * DS + j) = pre[i];
        }
        if (threadIdx.x < NEAREST_STAGE) {
            ra[threadIdx.x] = pa;
            rrel[threadIdx.x] = prel;
        }
        __syncthreads();
        if (m0 + NEAREST_STAGE < r1) fetch(m0 + NEAREST_STAGE);
#pragma unroll 1
        for (int t = 0; t < NEAREST_STAGE / 32; t++) {
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
            const float* arow = cs + (t * 32 + col) * DS + h * H;
#pragma unroll
            for (int s = 0; s < H; s += 4) {
                const float4 a = *reinterpret_cast<const float4*>(arow + s);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[s + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[s + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[s + 3], acc, 0, 0, 0);
            }
            // register 4g + q holds row ml = t * 32 + 8g + 4h + q of the step (D row), column col
#pragma unroll
            for (int g = 0; g < 4; g++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int ml = t * 32 + 8 * g + 4 * h + q;
                    const float av = ra[ml];
                    const float e = qc + rrel[ml];
                    float v, E;
                    if (COS) {
                        v = 1.f - acc[4 * g + q] * av * qa;
                        E = e;
                    } else {
                        const float S = av + qa;
                        v = fmaf(-2.f, acc[4 * g + q], S);
                        E = e * S;
                    }
                    const bool real = alive && av >= 0.f;
                    if (PASS == 1) {
                        const float hi = v + E;
                        mn = real ? fminf(mn, hi) : mn;
                    } else if (real && nearest_key(v - E) <= T) {
                        const int slot = atomicAdd(&kept.cnt[uq], 1);
                        if (slot < kept.cap) kept.krow[(size_t)uq * kept.cap + slot] = (int32_t)(m0 + ml);
                    }
                }
            }
            if (PASS == 1) {
                // the tile's 32 rows end a group (groups are whole tiles), or the segment
                const int64_t mt = m0 + t * 32;
                if (mt < r1 && (((mt + 32) & grp_mask) == 0 || mt + 32 >= r1)) {
                    const float w = fminf(mn, __shfl_xor(mn, 32));
                    const int64_t grp = mt >> kept.grp_shift;
                    if (alive && h == 0 && w < __builtin_inff() && grp < kept.groups)
                        kept.gkey[(size_t)uq * kept.groups + grp] = nearest_key(w);
                    mn = __builtin_inff();
                }
            }
        }
        __syncthreads();
    }
}

// One wave per query: tau = the k-th smallest of its group keys (a bitwise
// search for the largest value that fewer than k keys lie below); all ones when
// fewer than k groups hold a real row.
__global__ __launch_bounds__(256) void knn_select_kernel(KnnKept kept, int64_t nq) {
    constexpr int PER = KNN_GROUPS_MAX / 64;
    const int lane = threadIdx.x & 63;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += (int64_t)gridDim.x * 4) {
        uint32_t key[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int g = lane + 64 * i;
            key[i] = g < kept.groups ? kept.gkey[(size_t)q * kept.groups + g] : KNN_NO_KEY;
        }
        uint32_t ans = 0u;
        for (int bit = 31; bit >= 0; bit--) {
            const uint32_t cand = ans | (1u << bit);
            int below = 0;
#pragma unroll
            for (int i = 0; i < PER; i++) below += __popcll(__ballot(key[i] < cand));
            if (below < kept.k) ans = cand;
        }
        if (lane == 0) kept.tau[q] = ans;
    }
}

// An element of a query's list: ord orders the distances (numbers ascending
// with -0.0 = 0.0, then the NaNs, then the empty slots), key breaks ties.
struct KnnSlot {
    uint64_t ord;
    int64_t key;
    double v;
    int32_t row;
};
constexpr uint64_t KNN_ORD_NAN = 0xFFFFFFFFFFFFFFFEull, KNN_ORD_EMPTY = 0xFFFFFFFFFFFFFFFFull;
constexpr int64_t KNN_KEY_EMPTY = (int64_t)1 << 62;         // above every row and list position
__device__ inline KnnSlot knn_empty(int id) { return KnnSlot{KNN_ORD_EMPTY, KNN_KEY_EMPTY + id, 0.0, -1}; }
__device__ inline KnnSlot knn_slot(double v, int64_t key, int32_t row) {
    uint64_t u = (uint64_t)__double_as_longlong(v);
    if (v == 0.0) u = 0ull;
    const uint64_t ord = v != v ? KNN_ORD_NAN : (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return KnnSlot{ord, key, v, row};
}
__device__ inline bool knn_less(uint64_t ao, int64_t ak, uint64_t bo, int64_t bk) {
    return ao < bo || (ao == bo && ak < bk);
}

// A wave's sorted list of 64, slot `lane` in each lane's registers, and the LDS
// it merges through. Elements are distinct under (ord, key): the keys of a
// query's elements are distinct, the list's empty slots carry ids 0..63, a
// batch's 64..127.
struct KnnLds {
    uint64_t ord[128];
    int64_t key[128];
    double v[64];
    int32_t row[64];
};
// Merge the wave's batch (cand per lane) into its list (mine per lane): each
// element's rank among the 128 is the number of elements below it; ranks 0..63
// stay. Every lane of the wave calls it together.
__device__ inline void knn_merge(KnnSlot& mine, const KnnSlot& cand, KnnLds& s, int lane) {
    s.ord[lane] = mine.ord;
    s.key[lane] = mine.key;
    s.ord[64 + lane] = cand.ord;
    s.key[64 + lane] = cand.key;
    wave_sync();
    int ro = lane, rn = 0;                   // the list is sorted: `lane` of its elements lie below mine
    for (int j = 0; j < 64; j++) {
        const uint64_t no = s.ord[64 + j], oo = s.ord[j];
        const int64_t nk = s.key[64 + j], ok = s.key[j];
        ro += knn_less(no, nk, mine.ord, mine.key) ? 1 : 0;
        rn += (knn_less(no, nk, cand.ord, cand.key) ? 1 : 0) + (knn_less(oo, ok, cand.ord, cand.key) ? 1 : 0);
    }
    wave_sync();
    if (ro >= 0 && ro < 64) {
        s.ord[ro] = mine.ord;
        s.key[ro] = mine.key;
        s.v[ro] = mine.v;
        s.row[ro] = mine.row;
    }
    if (rn >= 0 && rn < 64) {
        s.ord[rn] = cand.ord;
        s.key[rn] = cand.key;
        s.v[rn] = cand.v;
        s.row[rn] = cand.row;
    }
    wave_sync();
    mine = KnnSlot{s.ord[lane], s.key[lane], s.v[lane], s.row[lane]};
    wave_sync();
}
// The batch joins the list unless none of it lies below the list's k-th.
__device__ inline void knn_take(KnnSlot& mine, const KnnSlot& cand, KnnLds& s, int lane, int k) {
    const uint64_t ko = __shfl(mine.ord, k - 1);
    const int64_t kk = __shfl(mine.key, k - 1);
    if (__any(knn_less(cand.ord, cand.key, ko, kk))) knn_merge(mine, cand, s, lane);
}
// Slot `lane` of query q's result (lanes < k): the first c slots hold elements.
__device__ inline void knn_store(const KnnSlot& mine, int lane, int k, int64_t c, int64_t q, int32_t* row_out,
                                 double* dist, int32_t* cnt_out) {
    if (lane < k) {
        row_out[(size_t)q * k + lane] = lane < c ? mine.row : -1;
        dist[(size_t)q * k + lane] = lane < c ? x86_nan(mine.v) : 0.0;
    }
    if (lane == 0 && cnt_out) cnt_out[q] = (int32_t)c;
}

// A query the screen leaves to the scan: a poison query, no tau, an overflow.
__device__ inline bool knn_handed(const KnnKept& kept, const float* __restrict__ qa, int64_t q) {
    return !(qa[q] >= 0.f) || kept.tau[q] == KNN_NO_KEY || kept.cnt[q] > kept.cap;
}

// One wave per query. Lists form (ptr != NULL): the caller's list
// idx[ptr[q] .. ptr[q+1]), key = the position. Kept form: the query's kept rows
// and the call's poison rows, key = the row; handed queries are the scan's.
template <typename T, int METRIC, bool LISTS>
__global__ __launch_bounds__(256) void knn_settle_kernel(const T* __restrict__ X, const T* __restrict__ Q, int64_t nq, int d,
                                                         int k, const int64_t* __restrict__ ptr,
                                                         const int32_t* __restrict__ idx, KnnKept kept,
                                                         const float* __restrict__ qa, const int32_t* __restrict__ pois,
                                                         const unsigned int* __restrict__ npois,
                                                         const double* __restrict__ xn2, const double* __restrict__ qn2,
                                                         int32_t* __restrict__ row_out, double* __restrict__ dist,
                                                         int32_t* __restrict__ cnt_out,
                                                         unsigned long long* __restrict__ stats) {
    __shared__ KnnLds lds[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = (int64_t)blockIdx.x * 4 + wave; q < nq; q += (int64_t)gridDim.x * 4) {
        int64_t b = 0, n = 0;
        int np = 0;
        if constexpr (LISTS) {
            b = ptr[q];
            n = ptr[q + 1] - b;
        } else {
            if (knn_handed(kept, qa, q)) continue;
            np = (int)min(*npois, (unsigned int)NEAREST_POISON_MAX);
            b = q * kept.cap;
            n = kept.cnt[q] + np;
        }
        KnnSlot mine = knn_empty(lane);
        const T* qv = Q + (size_t)q * d;
        double qn = -1.0;
        if constexpr (nearest_wants_norms<T, METRIC>()) qn = qn2[q];
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t i = base + lane;
            KnnSlot cand = knn_empty(64 + lane);
            if (i < n) {
                int32_t r;
                if constexpr (LISTS) r = idx[b + i];
                else r = i < n - np ? kept.krow[b + i] : pois[i - (n - np)];
                double xn = -1.0;
                if constexpr (nearest_wants_norms<T, METRIC>()) xn = xn2[r];
                cand = knn_slot(nearest_dist<T, METRIC>(qv, X + (size_t)r * d, d, qn, xn), LISTS ? i : (int64_t)r, r);
            }
            knn_take(mine, cand, lds[wave], lane, k);
        }
        knn_store(mine, lane, k, min(n, (int64_t)k), q, row_out, dist, cnt_out);
        if (lane == 0) atomicAdd(stats + STAT_KNN_EXACT, (unsigned long long)n);
    }
}

// The queries the screen hands to the scan, appended to list (any order).
__global__ __launch_bounds__(256) void knn_collect_kernel(KnnKept kept, const float* __restrict__ qa, int64_t nq,
                                                          int32_t* __restrict__ list, unsigned int* __restrict__ count,
                                                          unsigned long long* __restrict__ stats) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        const bool scan = knn_handed(kept, qa, q);
        if (scan) {
            const unsigned int slot = atomicAdd(count, 1u);
            if ((int64_t)slot < nq) list[slot] = (int32_t)q;
        }
        atomicAdd(stats + (scan ? STAT_KNN_SCAN : STAT_KNN_SETTLED), 1ull);
    }
}

// One block per query of list (NULL: every query) over all N rows: a list per
// wave, the four joined by wave 0.
template <typename T, int METRIC>
__global__ __launch_bounds__(256) void knn_scan_kernel(const T* __restrict__ X, int64_t N, const T* __restrict__ Q,
                                                       int64_t nq, int d, int k, const int32_t* __restrict__ list,
                                                       const unsigned int* __restrict__ count,
                                                       const double* __restrict__ xn2, const double* __restrict__ qn2,
                                                       int32_t* __restrict__ row_out, double* __restrict__ dist,
                                                       int32_t* __restrict__ cnt_out) {
    __shared__ KnnLds lds[4];
    __shared__ KnnSlot fin[3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = list ? min((int64_t)*count, nq) : nq;
    for (int64_t i = blockIdx.x; i < m; i += gridDim.x) {
        const int64_t q = list ? list[i] : i;
        const T* qv = Q + (size_t)q * d;
        double qn = -1.0;
        if constexpr (nearest_wants_norms<T, METRIC>()) qn = qn2[q];
        KnnSlot mine = knn_empty(lane);
        for (int64_t base = 0; base < N; base += 256) {
            const int64_t r = base + threadIdx.x;
            KnnSlot cand = knn_empty(64 + lane);
            if (r < N) {
                double xn = -1.0;
                if constexpr (nearest_wants_norms<T, METRIC>()) xn = xn2[r];
                cand = knn_slot(nearest_dist<T, METRIC>(qv, X + (size_t)r * d, d, qn, xn), r, (int32_t)r);
            }
            knn_take(mine, cand, lds[wave], lane, k);
        }
        if (wave > 0) fin[wave - 1][lane] = mine;
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < 3; w++) {
                KnnSlot cand = fin[w][lane];
                if (cand.ord == KNN_ORD_EMPTY) cand.key = KNN_KEY_EMPTY + 64 + lane;     // a batch's empty ids
                knn_take(mine, cand, lds[0], lane, k);
            }
            knn_store(mine, lane, k, min(N, (int64_t)k), q, row_out, dist, cnt_out);
        }
        __syncthreads();
    }
}

// N == 0: every slot row -1 and distance 0.0, every count 0.
__global__ __launch_bounds__(256) void knn_empty_kernel(int64_t nq, int k, int32_t* __restrict__ row_out,
                                                        double* __restrict__ dist, int32_t* __restrict__ cnt_out) {
    const int64_t total = nq * k;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        row_out[e] = -1;
        dist[e] = 0.0;
        if (cnt_out && e < nq) cnt_out[e] = 0;
    }
}

__global__ void knn_stats_kernel(unsigned long long* stats, unsigned long long scan) {
    if (threadIdx.x == 0 && blockIdx.x == 0) stats[STAT_KNN_SCAN] += scan;
}

template <int DP, bool COS>
static void knn_screen_passes(hipStream_t s, dim3 grid, const NearestSide& rows, const NearestSide& qs, const KnnKept& kept) {
    hipLaunchKernelGGL((knn_screen_kernel<DP, COS, 1>), grid, dim3(256), 0, s, rows, qs, kept);
    hipLaunchKernelGGL(knn_select_kernel, dim3(gsz(qs.n, 4, 16384)), dim3(256), 0, s, kept, qs.n);
    hipLaunchKernelGGL((knn_screen_kernel<DP, COS, 2>), grid, dim3(256), 0, s, rows, qs, kept);
}

int launch_knn_screen(hipStream_t s, int dp, int metric, const NearestSide& rows, const NearestSide& qs,
                      const KnnKept& kept, int64_t tiles, int segs) {
    if (qs.n <= 0 || rows.n <= 0) return 0;
    const int64_t grp_rows = (int64_t)1 << kept.grp_shift;
    if (kept.k < 1 || kept.k > KNN_KMAX || kept.cap < kept.k || tiles * NEAREST_COLS < qs.n || segs < 1 || segs > 65535 ||
        (int64_t)segs * kept.seg_rows < rows.n || kept.seg_rows % NEAREST_STAGE != 0 || kept.grp_shift < 5 ||
        kept.grp_shift > 31 || kept.seg_rows % grp_rows != 0 || kept.groups < kept.k || kept.groups > KNN_GROUPS_MAX ||
        (int64_t)kept.groups * grp_rows < rows.n || (dp != 32 && dp != 128)) {
        set_error("knn screen: unsupported shape");
        return -4;
    }
    if (hipMemsetAsync(kept.gkey, 0xff, 4 * (size_t)qs.n * kept.groups, s) != hipSuccess ||
        hipMemsetAsync(kept.cnt, 0, 4 * (size_t)qs.n, s) != hipSuccess) {
        set_error("knn screen: hipMemsetAsync failed");
        return -2;
    }
    const dim3 grid((unsigned)tiles, (unsigned)segs);
    const bool cos = metric == LSHKM_METRIC_COSINE;
    if (dp == 32) {
        if (cos) knn_screen_passes<32, true>(s, grid, rows, qs, kept);
        else knn_screen_passes<32, false>(s, grid, rows, qs, kept);
    } else {
        if (cos) knn_screen_passes<128, true>(s, grid, rows, qs, kept);
        else knn_screen_passes<128, false>(s, grid, rows, qs, kept);
    }
    return kstatus("knn_screen_kernel");
}

int launch_knn_settle(hipStream_t s, Pts X, Pts Q, int64_t nq, int d, int metric, int k, const int64_t* ptr,
                      const int32_t* idx, const KnnKept& kept, const float* qa, const int32_t* pois,
                      const unsigned int* npois, const double* xn2, const double* qn2, int32_t* row, double* dist,
                      int32_t* cnt, unsigned long long* stats) {
    if (nq <= 0) return 0;
    with_rows(X, [&](auto* x) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        const bool cos = metric == LSHKM_METRIC_COSINE;
        const auto kernel = ptr ? (cos ? knn_settle_kernel<T, LSHKM_METRIC_COSINE, true>
                                       : knn_settle_kernel<T, LSHKM_METRIC_EUCLIDEAN, true>)
                                : (cos ? knn_settle_kernel<T, LSHKM_METRIC_COSINE, false>
                                       : knn_settle_kernel<T, LSHKM_METRIC_EUCLIDEAN, false>);
        hipLaunchKernelGGL(kernel, dim3(gsz(nq, 4, 16384)), dim3(256), 0, s, x, static_cast<decltype(x)>(Q.p), nq, d, k,
                           ptr, idx, kept, qa, pois, npois, xn2, qn2, row, dist, cnt, stats);
    });
    return kstatus("knn_settle_kernel");
}

int launch_knn_collect(hipStream_t s, const KnnKept& kept, const float* qa, int64_t nq, int32_t* list,
                       unsigned int* count, unsigned long long* stats) {
    if (nq <= 0) return 0;
    hipLaunchKernelGGL(knn_collect_kernel, dim3(gsz(nq, 256, 1024)), dim3(256), 0, s, kept, qa, nq, list, count, stats);
    return kstatus("knn_collect_kernel");
}

int launch_knn_scan(hipStream_t s, Pts X, int64_t N, Pts Q, int64_t nq, int d, int metric, int k, const int32_t* list,
                    const unsigned int* count, const double* xn2, const double* qn2, int32_t* row, double* dist,
                    int32_t* cnt, unsigned long long* stats) {
    if (nq <= 0) return 0;
    with_rows(X, [&](auto* x) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        const auto kernel = metric == LSHKM_METRIC_COSINE ? knn_scan_kernel<T, LSHKM_METRIC_COSINE>
                                                          : knn_scan_kernel<T, LSHKM_METRIC_EUCLIDEAN>;
        hipLaunchKernelGGL(kernel, dim3(gsz(nq, 1, 8192)), dim3(256), 0, s, x, N, static_cast<decltype(x)>(Q.p), nq, d, k,
                           list, count, xn2, qn2, row, dist, cnt);
    });
    if (!list) hipLaunchKernelGGL(knn_stats_kernel, dim3(1), dim3(64), 0, s, stats, (unsigned long long)nq);
    return kstatus("knn_scan_kernel");
}

int launch_knn_empty(hipStream_t s, int64_t nq, int k, int32_t* row, double* dist, int32_t* cnt) {
    if (nq <= 0) return 0;
    hipLaunchKernelGGL(knn_empty_kernel, dim3(gsz(nq * k, 256, 1024)), dim3(256), 0, s, nq, k, row, dist, cnt);
    return kstatus("knn_empty_kernel");
}

}  // namespace lshkm
