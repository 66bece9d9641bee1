// nearest.hip — lshkm_min_vector_dist: the exact nearest row of
// every query, min_vector_euclidean_dist / min_vector_cosine_dist of
// lib/utils.hpp:107-140 for nq queries at once.
//
// The screen: a block owns NEAREST_COLS queries as the f32 32x32x2 MFMA's B
// operand (32 per wave, one column per lane pair, in registers) and walks one
// segment of the rows, NEAREST_STAGE at a time through LDS (the A operand;
// lsh_closest.hip's layout and row stride), the next step's rows fetched one
// step ahead. For every (query, row) pair it has a value v~ (euclidean: |q^|^2 +
// |x^|^2 - 2 g~, the squared distance; cosine: 1 - g~ / (|x^||q^|)) and a
// radius E with the reference's double (euclidean: the fp64 chain under its
// sqrt) inside [v~ - E, v~ + E] by a margin that survives the reference's last
// roundings (§5f). Two passes over the rows:
//   1. minkey[q] <- the smallest hi = v~ + E over the rows (register min, one
//      atomicMin of the order-preserving key per (query, segment));
//   2. the rows with lo = v~ - E <= that minimum are appended to the query's
//      kept rows (capacity cap; a longer list flags the query for the scan).
// Both passes compute the same v~ and E (the same instruction sequence on the
// same data), so the row that set the minimum is kept, and the kept set is a
// function of the inputs alone: minkey is final before pass 2 starts, and the
// settle orders by (value, row), not by arrival.
//
// The settle: one wave per query over its kept rows and the call's poison
// rows, the exact chains of exact.h, then the (value, lowest key) minimum under
// the reference's loop rule (start from the first, replace on strict <: a NaN
// is taken only as the first element). The same kernel serves the lists form
// (key = the position in the caller's list). The scan: one block per handed
// query over all N rows.
#include "../../include/lshkm.h"
#include "common.h"
#include "exact.h"
#include "kernels.h"
#include "nearest_layout.h"
#include "nearest_dev.h"

#include <type_traits>

namespace lshkm {

// Magnitude range the bound assumes for |x^|^2 (then no f32 operand, product or
// partial sum leaves the normal range by more than the 2^-40 term covers).
constexpr double NEAREST_S_MIN = 0x1p-40, NEAREST_S_MAX = 0x1p40;

// One wave per row: the f32 image x^ (zero-padded to dp), a = |x^|^2 (euclidean)
// or 1 / |x^| (cosine), negative: poison; rel = the conversion term, with eps =
// rho / |x^| (rho >= |x - x^|_2): 2.001 eps (cosine), 4.001 eps (euclidean).
// Poison: a non-finite entry or image, |x^|^2 outside the range above, a zero
// image under cosine or with a nonzero rest, eps >= 2^-12. pois (rows only):
// the poison rows' list, *npois their count (entries past NEAREST_POISON_MAX
// are counted, not written).
template <typename T>
__global__ __launch_bounds__(256) void nearest_prep_kernel(const T* __restrict__ X, int64_t n, int d, int dp, int metric,
                                                           float* __restrict__ xh, float* __restrict__ a,
                                                           float* __restrict__ rel, int32_t* __restrict__ pois,
                                                           unsigned int* __restrict__ npois) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
        double s = 0.0, rr = 0.0;
        bool bad = false, rest = false;          // rest: x^ != x (rr itself may underflow to 0)
        for (int j = lane; j < dp; j += 64) {
            const double v = j < d ? (double)X[(size_t)r * d + j] : 0.0;
            const float f = (float)v;
            const double fd = (double)f, dl = v - fd;
            bad |= !(fabs(v) < __builtin_inf()) || !(fabsf(f) < __builtin_inff());
            rest |= dl != 0.0;
            xh[(size_t)r * dp + j] = f;
            s = fma(fd, fd, s);
            rr = fma(dl, dl, rr);
        }
        for (int off = 32; off >= 1; off >>= 1) {
            s += __shfl_xor(s, off);
            rr += __shfl_xor(rr, off);
        }
        bad = __any(bad);
        rest = __any(rest);
        double relv = 0.0;
        if (s > 0.0) {
            bad |= !(s >= NEAREST_S_MIN && s <= NEAREST_S_MAX);
            const double eps = (sqrt(rr) * (1.0 + 0x1p-20)) / sqrt(s);
            bad |= !(eps < 0x1p-12);
            relv = (metric == LSHKM_METRIC_COSINE ? 2.001 : 4.001) * eps;
        } else {
            bad |= !(s == 0.0) || metric == LSHKM_METRIC_COSINE || rest;
        }
        if (lane == 0) {
            const double av = metric == LSHKM_METRIC_COSINE ? 1.0 / sqrt(s) : s;
            a[r] = bad ? -1.f : (float)av;
            rel[r] = bad ? 0.f : (float)relv * (1.f + 0x1p-20f);
            if (bad && npois) {
                const unsigned int slot = atomicAdd(npois, 1u);
                if (slot < (unsigned int)NEAREST_POISON_MAX) pois[slot] = (int32_t)r;
            }
        }
    }
}

// PASS 1: minkey; PASS 2: the kept rows.
template <int DP, bool COS, int PASS>
__global__ __launch_bounds__(256, 2) void nearest_screen_kernel(NearestSide rows, NearestSide qs, NearestKept kept) {
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
    const bool alive = own && qa >= 0.f;
    uint32_t T = 0u;
    if (PASS == 2 && alive) T = kept.minkey[uq];
    float mn = __builtin_inff();
    const int64_t r0 = (int64_t)blockIdx.y * kept.seg_rows, r1 = min(rows.n, r0 + kept.seg_rows);
    // A step's rows are fetched into registers one step ahead (the loads fly
    // under the previous step's MFMAs) and stored to LDS at the step's top.
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
        }
        __syncthreads();
    }
    if (PASS == 1) {
        mn = fminf(mn, __shfl_xor(mn, 32));
        if (alive && h == 0 && mn < __builtin_inff()) atomicMin(&kept.minkey[uq], nearest_key(mn));
    }
}

// The reference's loop over one list, a lane's share: (v, key) replaces the
// lane's best on v < best, or v == best at a lower key; a NaN never does.
struct NearestBest {
    double v, nan_v;     // the smallest non-NaN value; the NaN of the element of key 0
    int64_t key;
    int32_t row, nan_row;
    bool first_nan;      // the element of key 0 is a NaN: the list's answer
    __device__ inline void init() {
        v = __builtin_inf();
        nan_v = 0.0;
        key = INT64_MAX;
        row = nan_row = -1;
        first_nan = false;
    }
    __device__ inline void take(double nv, int64_t nkey, int32_t nrow) {
        if (nv != nv) {
            if (nkey == 0) {
                first_nan = true;
                nan_v = nv;
                nan_row = nrow;
            }
        } else if (nv < v || (nv == v && nkey < key)) {
            v = nv;
            key = nkey;
            row = nrow;
        }
    }
    __device__ inline void join(double ov, int64_t ok, int32_t orow, bool ofn, double onv, int32_t onrow) {
        if (ofn) {
            first_nan = true;
            nan_v = onv;
            nan_row = onrow;
        }
        if (ov < v || (ov == v && ok < key)) {
            v = ov;
            key = ok;
            row = orow;
        }
    }
    // the wave's lanes joined; every lane ends with the result
    __device__ inline void join_wave() {
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(v, off), onv = __shfl_xor(nan_v, off);
            const int64_t ok = __shfl_xor(key, off);
            const int32_t orow = __shfl_xor(row, off), onrow = __shfl_xor(nan_row, off);
            const bool ofn = __shfl_xor((int)first_nan, off) != 0;
            join(ov, ok, orow, ofn, onv, onrow);
        }
    }
    __device__ inline void store(bool empty, double* dist, int32_t* row_out, int64_t q) const {
        dist[q] = empty ? 0.0 : first_nan ? x86_nan(nan_v) : v;
        if (row_out) row_out[q] = empty ? -1 : first_nan ? nan_row : row;
    }
};

// One wave per query. Lists form (ptr != NULL): the caller's list
// idx[ptr[q] .. ptr[q+1]), key = the position. Kept form: the query's kept rows
// and the call's poison rows, key = the row; queries the screen flagged (a
// poison query, an overflow) are left to the scan.
template <typename T, int METRIC, bool LISTS>
__global__ __launch_bounds__(256) void nearest_settle_kernel(const T* __restrict__ X, const T* __restrict__ Q, int64_t nq,
                                                             int d, const int64_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ idx, NearestKept kept,
                                                             const float* __restrict__ qa,
                                                             const int32_t* __restrict__ pois,
                                                             const unsigned int* __restrict__ npois,
                                                             const double* __restrict__ xn2,
                                                             const double* __restrict__ qn2,
                                                             double* __restrict__ dist, int32_t* __restrict__ row_out,
                                                             unsigned long long* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += (int64_t)gridDim.x * 4) {
        int64_t b = 0, n = 0;
        int np = 0;
        if constexpr (LISTS) {
            b = ptr[q];
            n = ptr[q + 1] - b;
        } else {
            const int c = kept.cnt[q];
            if (!(qa[q] >= 0.f) || c > kept.cap) continue;
            np = (int)min(*npois, (unsigned int)NEAREST_POISON_MAX);
            b = q * kept.cap;
            n = c + np;
        }
        NearestBest best;
        best.init();
        const T* qv = Q + (size_t)q * d;
        double qn = -1.0;
        if constexpr (nearest_wants_norms<T, METRIC>()) qn = qn2[q];
        for (int64_t i = lane; i < n; i += 64) {
            int32_t r;
            if constexpr (LISTS) r = idx[b + i];
            else r = i < n - np ? kept.krow[b + i] : pois[i - (n - np)];
            double xn = -1.0;
            if constexpr (nearest_wants_norms<T, METRIC>()) xn = xn2[r];
            const double v = nearest_dist<T, METRIC>(qv, X + (size_t)r * d, d, qn, xn);
            best.take(v, LISTS ? i : (int64_t)r, r);
        }
        best.join_wave();
        if (lane == 0) {
            best.store(n == 0, dist, row_out, q);
            atomicAdd(stats + STAT_NEAREST_EXACT, (unsigned long long)n);
        }
    }
}

// The queries the screen hands to the scan, appended to list (any order).
__global__ __launch_bounds__(256) void nearest_collect_kernel(NearestKept kept, const float* __restrict__ qa, int64_t nq,
                                                              int32_t* __restrict__ list, unsigned int* __restrict__ count,
                                                              unsigned long long* __restrict__ stats) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        const bool scan = !(qa[q] >= 0.f) || kept.cnt[q] > kept.cap;
        if (scan) list[atomicAdd(count, 1u)] = (int32_t)q;
        atomicAdd(stats + (scan ? STAT_NEAREST_SCAN : STAT_NEAREST_SETTLED), 1ull);
    }
}

// One block per query of list (NULL: every query) over all N rows.
template <typename T, int METRIC>
__global__ __launch_bounds__(256) void nearest_scan_kernel(const T* __restrict__ X, int64_t N, const T* __restrict__ Q,
                                                           int64_t nq, int d, const int32_t* __restrict__ list,
                                                           const unsigned int* __restrict__ count,
                                                           const double* __restrict__ xn2,
                                                           const double* __restrict__ qn2, double* __restrict__ dist,
                                                           int32_t* __restrict__ row_out) {
    __shared__ double sv[4], snv[4];
    __shared__ int64_t sk[4];
    __shared__ int32_t srow[4], snrow[4];
    __shared__ int sfn[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = list ? (int64_t)*count : nq;
    for (int64_t i = blockIdx.x; i < m; i += gridDim.x) {
        const int64_t q = list ? list[i] : i;
        const T* qv = Q + (size_t)q * d;
        double qn = -1.0;
        if constexpr (nearest_wants_norms<T, METRIC>()) qn = qn2[q];
        NearestBest best;
        best.init();
        for (int64_t r = threadIdx.x; r < N; r += 256) {
            double xn = -1.0;
            if constexpr (nearest_wants_norms<T, METRIC>()) xn = xn2[r];
            best.take(nearest_dist<T, METRIC>(qv, X + (size_t)r * d, d, qn, xn), r, (int32_t)r);
        }
        best.join_wave();
        if (lane == 0) {
            sv[wave] = best.v;
            snv[wave] = best.nan_v;
            sk[wave] = best.key;
            srow[wave] = best.row;
            snrow[wave] = best.nan_row;
            sfn[wave] = best.first_nan;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) best.join(sv[w], sk[w], srow[w], sfn[w] != 0, snv[w], snrow[w]);
            best.store(N == 0, dist, row_out, q);
        }
        __syncthreads();
    }
}

// N == 0 or an empty call: dist = 0.0, row = -1 (utils.hpp:109-110).
__global__ __launch_bounds__(256) void nearest_empty_kernel(int64_t nq, double* __restrict__ dist,
                                                            int32_t* __restrict__ row_out) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        dist[q] = 0.0;
        if (row_out) row_out[q] = -1;
    }
}

// The lists form's argument check: *bad <- 1 on a decreasing ptr or an index
// outside [0, N).
__global__ __launch_bounds__(256) void nearest_check_kernel(const int64_t* __restrict__ ptr, int64_t nq,
                                                            const int32_t* __restrict__ idx, int64_t total, int64_t N,
                                                            unsigned int* __restrict__ bad) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    bool b = false;
    for (int64_t q = t0; q < nq; q += step) b |= ptr[q + 1] < ptr[q] || (q == 0 && ptr[0] != 0);
    for (int64_t e = t0; e < total; e += step) b |= idx[e] < 0 || idx[e] >= N;
    if (b) *bad = 1u;
}

__global__ void nearest_stats_kernel(unsigned long long* stats, unsigned long long scan) {
    if (threadIdx.x == 0 && blockIdx.x == 0) stats[STAT_NEAREST_SCAN] += scan;
}

int launch_nearest_prep(hipStream_t s, Pts X, int64_t n, int d, int dp, int metric, const NearestSide& out, int32_t* pois,
                        unsigned int* npois) {
    if (n <= 0) return 0;
    with_rows(X, [&](auto* x) {
        hipLaunchKernelGGL(nearest_prep_kernel, dim3(gsz(n, 4, 8192)), dim3(256), 0, s, x, n, d, dp, metric,
                           const_cast<float*>(out.xh), const_cast<float*>(out.a), const_cast<float*>(out.rel), pois,
                           npois);
    });
    return kstatus("nearest_prep_kernel");
}

template <int DP, bool COS>
static void screen_passes(hipStream_t s, dim3 grid, const NearestSide& rows, const NearestSide& qs, const NearestKept& kept) {
    hipLaunchKernelGGL((nearest_screen_kernel<DP, COS, 1>), grid, dim3(256), 0, s, rows, qs, kept);
    hipLaunchKernelGGL((nearest_screen_kernel<DP, COS, 2>), grid, dim3(256), 0, s, rows, qs, kept);
}

int launch_nearest_screen(hipStream_t s, int dp, int metric, const NearestSide& rows, const NearestSide& qs,
                          const NearestKept& kept, int64_t tiles, int segs) {
    if (qs.n <= 0 || rows.n <= 0) return 0;
    if (kept.cap < NEAREST_CAP_MIN || tiles * NEAREST_COLS < qs.n || segs < 1 || segs > 65535 ||
        (int64_t)segs * kept.seg_rows < rows.n || kept.seg_rows % NEAREST_STAGE != 0 || (dp != 32 && dp != 128)) {
        set_error("nearest screen: unsupported shape");
        return -4;
    }
    if (hipMemsetAsync(kept.minkey, 0xff, 4 * (size_t)qs.n, s) != hipSuccess ||
        hipMemsetAsync(kept.cnt, 0, 4 * (size_t)qs.n, s) != hipSuccess) {
        set_error("nearest screen: hipMemsetAsync failed");
        return -2;
    }
    const dim3 grid((unsigned)tiles, (unsigned)segs);
    const bool cos = metric == LSHKM_METRIC_COSINE;
    if (dp == 32) {
        if (cos) screen_passes<32, true>(s, grid, rows, qs, kept);
        else screen_passes<32, false>(s, grid, rows, qs, kept);
    } else {
        if (cos) screen_passes<128, true>(s, grid, rows, qs, kept);
        else screen_passes<128, false>(s, grid, rows, qs, kept);
    }
    return kstatus("nearest_screen_kernel");
}

int launch_nearest_settle(hipStream_t s, Pts X, Pts Q, int64_t nq, int d, int metric, const int64_t* ptr,
                          const int32_t* idx, const NearestKept& kept, const float* qa, const int32_t* pois,
                          const unsigned int* npois, const double* xn2, const double* qn2, double* dist, int32_t* row,
                          unsigned long long* stats) {
    if (nq <= 0) return 0;
    with_rows(X, [&](auto* x) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        const bool cos = metric == LSHKM_METRIC_COSINE;
        const auto kernel = ptr ? (cos ? nearest_settle_kernel<T, LSHKM_METRIC_COSINE, true>
                                       : nearest_settle_kernel<T, LSHKM_METRIC_EUCLIDEAN, true>)
                                : (cos ? nearest_settle_kernel<T, LSHKM_METRIC_COSINE, false>
                                       : nearest_settle_kernel<T, LSHKM_METRIC_EUCLIDEAN, false>);
        hipLaunchKernelGGL(kernel, dim3(gsz(nq, 4, 16384)), dim3(256), 0, s, x, static_cast<decltype(x)>(Q.p), nq, d, ptr,
                           idx, kept, qa, pois, npois, xn2, qn2, dist, row, stats);
    });
    return kstatus("nearest_settle_kernel");
}

int launch_nearest_collect(hipStream_t s, const NearestKept& kept, const float* qa, int64_t nq, int32_t* list,
                           unsigned int* count, unsigned long long* stats) {
    if (nq <= 0) return 0;
    hipLaunchKernelGGL(nearest_collect_kernel, dim3(gsz(nq, 256, 1024)), dim3(256), 0, s, kept, qa, nq, list, count,
                       stats);
    return kstatus("nearest_collect_kernel");
}

int launch_nearest_scan(hipStream_t s, Pts X, int64_t N, Pts Q, int64_t nq, int d, int metric, const int32_t* list,
                        const unsigned int* count, const double* xn2, const double* qn2, double* dist, int32_t* row,
                        unsigned long long* stats) {
    if (nq <= 0) return 0;
    with_rows(X, [&](auto* x) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        const auto kernel = metric == LSHKM_METRIC_COSINE ? nearest_scan_kernel<T, LSHKM_METRIC_COSINE>
                                                          : nearest_scan_kernel<T, LSHKM_METRIC_EUCLIDEAN>;
        hipLaunchKernelGGL(kernel, dim3(gsz(nq, 1, 8192)), dim3(256), 0, s, x, N, static_cast<decltype(x)>(Q.p), nq, d,
                           list, count, xn2, qn2, dist, row);
    });
    if (!list) hipLaunchKernelGGL(nearest_stats_kernel, dim3(1), dim3(64), 0, s, stats, (unsigned long long)nq);
    return kstatus("nearest_scan_kernel");
}

// The reference's sums of squares, where the exact chains want them given
// (cosine on fp64 values): xa [n], else nothing.
bool nearest_needs_norms(Pts X, int metric) { return X.f64 && metric == LSHKM_METRIC_COSINE; }
int launch_nearest_norms(hipStream_t s, Pts X, int64_t n, int d, int metric, double* xa) {
    if (n <= 0 || !nearest_needs_norms(X, metric)) return 0;
    return launch_rc_norms(s, X.d(), n, d, xa);
}

int launch_nearest_empty(hipStream_t s, int64_t nq, double* dist, int32_t* row) {
    if (nq <= 0) return 0;
    hipLaunchKernelGGL(nearest_empty_kernel, dim3(gsz(nq, 256, 1024)), dim3(256), 0, s, nq, dist, row);
    return kstatus("nearest_empty_kernel");
}

int launch_nearest_check(hipStream_t s, const int64_t* ptr, int64_t nq, const int32_t* idx, int64_t total, int64_t N,
                         unsigned int* bad) {
    hipLaunchKernelGGL(nearest_check_kernel, dim3(gsz(std::max(nq, total), 256, 4096)), dim3(256), 0, s, ptr, nq, idx,
                       total, N, bad);
    return kstatus("nearest_check_kernel");
}

}  // namespace lshkm
