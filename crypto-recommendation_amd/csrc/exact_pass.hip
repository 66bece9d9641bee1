// exact_pass.hip — the listed exact pass: the rows no certificate decided,
// finished in the reference's exact order (lloyds_assignment,
// lib/clustering_phases/assignment.hpp:54-80: every centroid, strict '<', the
// first minimum wins). Four forms, chosen by exact_route (exact_layout.h):
// every, batch, pruned, pruned_wide. One launcher each for the centroid-only
// prep and for the pass.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "exact.h"
#include "pick.h"
#include "settle.h"

namespace lshkm {

// ------------------------------------------------------------ shared pieces
// The part of a list a wave walks, in groups of R rows (R = 1: rows): group
// g0, g0 + gstride, ... of rows[0, total). A flat list (or, rows == NULL, every
// row below max_rows) is dealt over the whole grid; of a segmented one, SPLIT
// blocks of WAVES waves share each segment (block b -> segment b % nseg: the
// segments across XCDs, as cos_fix_seg_kernel).
struct ListWalk {
    const int32_t* rows;
    int64_t total, g0, gstride;
};
template <int SPLIT, int WAVES>
__device__ inline ListWalk list_walk(const int32_t* rows, const unsigned long long* row_count, int64_t max_rows,
                                     const int32_t* seg_counts, int64_t seg_rows) {
    const int wave = threadIdx.x >> 6;
    ListWalk w;
    if (seg_counts) {
        const int nseg = gridDim.x / SPLIT;
        const int seg = blockIdx.x % nseg, part = blockIdx.x / nseg;
        w.rows = rows + (int64_t)seg * seg_rows;
        w.total = seg_counts[SEG_SLOTS * seg + SEG_ROWS];
        w.g0 = (int64_t)part * WAVES + wave;
        w.gstride = (int64_t)SPLIT * WAVES;
    } else {
        w.rows = rows;
        w.total = rows ? (int64_t)*row_count : max_rows;
        w.g0 = (int64_t)blockIdx.x * WAVES + wave;
        w.gstride = (int64_t)gridDim.x * WAVES;
    }
    if (w.total > max_rows) w.total = max_rows;
    return w;
}

// The R rows of the group at rows[base..] of a list of cnt rows, padded with
// the last one; returns how many are the group's own.
template <int R>
__device__ inline int group_rows(const int32_t* __restrict__ rows, int64_t base, int64_t cnt, int32_t (&myrow)[R]) {
    const int nr = (int)min((int64_t)R, cnt - base);
#pragma unroll
    for (int r = 0; r < R; r++) myrow[r] = rows[base + min(r, nr - 1)];
    return nr;
}

// Stages the group's rows in LDS (d <= XB_DMAX): every row value of the group
// in flight at once, at most XB_DMAX / 64 per lane and row. xn2p: the lane's
// f32 partial sum of squares of each row.
template <int R, typename TX>
__device__ inline void stage_rows(const TX* __restrict__ X, int d, const int32_t (&myrow)[R], TX (*xs)[XB_DMAX],
                                  float (&xn2p)[R]) {
    const int lane = threadIdx.x & 63;
    TX xv[R][XB_DMAX / 64];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int u = 0; u < XB_DMAX / 64; u++) {
            const int j = lane + 64 * u;
            xv[r][u] = j < d ? X[(int64_t)myrow[r] * d + j] : TX(0);
        }
#pragma unroll
    for (int r = 0; r < R; r++) {
        float q = 0.f;
#pragma unroll
        for (int u = 0; u < XB_DMAX / 64; u++) {
            const int j = lane + 64 * u;
            if (j < d) {
                xs[r][j] = xv[r][u];
                q = fmaf((float)xv[r][u], (float)xv[r][u], q);
            }
        }
        xn2p[r] = q;
    }
    wave_sync();
}

// Cosine, a row with an inf or NaN entry: every product with it is inf or NaN
// and the row's norm is, so every distance is the default NaN (inf / inf) and
// the sentinel keeps centroid 0. The soft-x87 chains take finite products only
// (softx87.h), so such a row is decided here. True: (best, bi) set.
template <typename TX>
__device__ inline bool cosine_nonfinite_row(const TX* x, int d, double& best, int& bi) {
    bool bad = false;
    for (int j = threadIdx.x & 63; j < d; j += 64) bad |= !(fabs((double)x[j]) <= 1.7976931348623157e308);
    if (!__any(bad)) return false;
    best = __longlong_as_double((long long)0xFFF8000000000000ull);
    bi = 0;
    return true;
}

// -------------------------------------------------------------------- every
constexpr int XC_MAXV = 4;   // cosine candidate form: K <= 256 (values kept per lane)
// One wave per listed row; lane c evaluates centroids c, c+64, ... in the
// reference's exact order (exact.h).
template <typename TX>
__global__ __launch_bounds__(64 * XE_WAVES) void assign_exact_kernel(
    const TX* __restrict__ X, int d, const double* __restrict__ C, int K, int metric,
    const int32_t* __restrict__ rows, const unsigned long long* __restrict__ row_count, int64_t max_rows,
    int32_t* __restrict__ assign, double* __restrict__ dist, const int32_t* __restrict__ seg_counts,
    int64_t seg_rows, const double* __restrict__ xn2, const double* __restrict__ nbv) {
    const int lane = threadIdx.x & 63;
    const ListWalk w = list_walk<XE_SPLIT, XE_WAVES>(rows, row_count, max_rows, seg_counts, seg_rows);
    for (int64_t it = w.g0; it < w.total; it += w.gstride) {
        const int64_t row = w.rows ? w.rows[it] : it;
        const TX* x = X + row * d;
        double best = 0.0; int bi = -1;
        // cosine: the row's / centroids' sums of squares precomputed (row_sumsq,
        // the prep's nbv; glibc pow per square, the same for every pair) when given
        const double xa = metric == 1 && xn2 ? xn2[row] : -1.0;
        if (metric == 1 && cosine_nonfinite_row(x, d, best, bi)) {
            wave_store(best, bi, row, assign, dist);
            continue;
        }
        if (metric == 1 && K <= 64 * XC_MAXV) {
            // cosine: certified values (exact.h cosine_interval) for every
            // centroid, the soft-x87 chain only for those whose interval can
            // still reach the minimum; a row with an unknown value (zero
            // vectors, NaN/inf, extreme ranges) takes the full soft pass below
            double v[XC_MAXV], rad[XC_MAXV];
            int st[XC_MAXV];
            double U = __builtin_inf();
            bool unknown = false;
#pragma unroll
            for (int k = 0; k < XC_MAXV; k++) {
                const int c = lane + 64 * k;
                st[k] = 0; v[k] = 0.0; rad[k] = 0.0;
                if (c < K) {
                    st[k] = cosine_interval(x, C + (size_t)c * d, d, v[k], rad[k], xa, nbv ? nbv[c] : -1.0);
                    unknown |= st[k] == 2;
                    if (st[k] != 2) U = fmin(U, v[k] + rad[k]);
                }
            }
            if (!__ballot(unknown)) {
                U = group_min<64>(U);
#pragma unroll
                for (int k = 0; k < XC_MAXV; k++) {
                    const int c = lane + 64 * k;
                    if (c < K && v[k] - rad[k] <= U) {     // non-candidates are strictly above the minimum
                        const double dd = st[k] == 0 ? v[k] : exact_cosine_x87(x, C + (size_t)c * d, d, xa, nbv ? nbv[c] : -1.0);
                        if (bi < 0 || dd < best) { best = dd; bi = c; }
                    }
                }
                group_argmin<64>(best, bi);
                if (lane == 0) {
                    assign[row] = bi;
                    dist[row] = best;
                }
                continue;
            }
        }
        every_centroid(K, [&](int c) {
            return metric == 0 ? exact_euclid(x, C + (size_t)c * d, d)
                               : exact_cosine_x87(x, C + (size_t)c * d, d, xa, nbv ? nbv[c] : -1.0);
        }, best, bi);
        wave_store(best, bi, row, assign, dist);
    }
}

// -------------------------------------------------------------------- batch
// Euclidean: the same reference-order distances as assign_exact_kernel, but a
// wave takes XB_R rows at once against a transposed fp64 copy CT[j][c], so each
// centroid value is loaded once (coalesced, lane = centroid) for XB_R rows.
// Lane holds centroids c0 + lane + 64i, i < 4.
__global__ void transpose_centroids_kernel(const double* __restrict__ C, int K, int Kpad, int d,
                                           double* __restrict__ CT) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)d * Kpad) return;
    const int j = (int)(e / Kpad), c = (int)(e % Kpad);
    CT[e] = c < K ? C[(size_t)c * d + j] : 0.0;
}

template <typename TX>
__global__ __launch_bounds__(64 * XB_WAVES) void assign_exact_batch_kernel(
    const TX* __restrict__ X, int d, const double* __restrict__ CT, int K, int Kpad,
    const int32_t* __restrict__ rows, const unsigned long long* __restrict__ row_count, int64_t max_rows,
    int32_t* __restrict__ assign, double* __restrict__ dist, const int32_t* __restrict__ seg_counts,
    int64_t seg_rows) {
    __shared__ TX xs[XB_WAVES][XB_R][XB_DMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ListWalk w = list_walk<XB_SPLIT, XB_WAVES>(rows, row_count, max_rows, seg_counts, seg_rows);
    const int64_t ngroups = (w.total + XB_R - 1) / XB_R;
    for (int64_t g = w.g0; g < ngroups; g += w.gstride) {
        int32_t myrow[XB_R];
        const int nr = group_rows(w.rows, g * XB_R, w.total, myrow);
        float xn2p[XB_R];
        stage_rows(X, d, myrow, xs[wave], xn2p);
        double best[XB_R];
        int bi[XB_R];
#pragma unroll
        for (int r = 0; r < XB_R; r++) { best[r] = 0.0; bi[r] = -1; }
        for (int c0 = 0; c0 < K; c0 += 256) {
            double acc[XB_R][4];
#pragma unroll
            for (int r = 0; r < XB_R; r++)
#pragma unroll
                for (int i = 0; i < 4; i++) acc[r][i] = 0.0;
            const double* ct = CT + c0 + lane;   // CT rows are padded to a multiple of 256 columns
#pragma unroll 4
            for (int j = 0; j < d; j++) {
                double cv[4];
#pragma unroll
                for (int i = 0; i < 4; i++) cv[i] = ct[(size_t)j * Kpad + 64 * i];
#pragma unroll
                for (int r = 0; r < XB_R; r++) {
                    const double xj = (double)xs[wave][r][j];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const double df = __dsub_rn(xj, cv[i]);
                        acc[r][i] = __dadd_rn(acc[r][i], gp_sq(df));
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {           // increasing c: strict '<' keeps the first minimum
                const int c = c0 + lane + 64 * i;
                if (c >= K) continue;
#pragma unroll
                for (int r = 0; r < XB_R; r++) {
                    const double dd = sqrt(acc[r][i]);
                    if (bi[r] < 0 || dd < best[r]) { best[r] = dd; bi[r] = c; }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < XB_R; r++) {
            double b = best[r];
            int i1 = bi[r];
            group_argmin<64>(b, i1);
            if (lane == 0 && r < nr) {
                assign[myrow[r]] = i1;
                dist[myrow[r]] = b;
            }
        }
        wave_sync();
    }
}

// ------------------------------------------------------------------- pruned
// K <= XP_KMAX: a wave takes R rows; phase 1 scores every centroid in f32 (an
// FMA chain over a transposed f32 copy CT32[j][c], loaded once per R rows) with
// the bound e_c of the f32-MFMA path (assign.hip); the candidates are the
// centroids with s~_c - e_c <= min (s~ + e) -- every other centroid's reference
// distance is provably larger than some candidate's -- and phase 2 evaluates
// only those in the reference's exact order (one lane each), keeping the first
// minimum. A row whose f32 scores are not all finite, or with more than 64
// candidates, evaluates every centroid exactly instead.

// The reference's distance of one (row, centroid) pair on the pruned pass:
// euclidean in exact order; cosine by the soft-x87 chain (16-B loads when the
// row length allows).
template <int MET, typename TX>
__device__ inline double pruned_dist(const TX* __restrict__ x, const double* __restrict__ c, int d) {
    if constexpr (MET == 0) {
        return exact_euclid_rolled(x, c, d);
    } else {
        if constexpr (sizeof(TX) == 4) {
            if ((d & 15) == 0) return exact_cosine_x87_b16(x, c, d);
        }
        return exact_cosine_x87(x, c, d);
    }
}

__global__ void exact_prep_kernel(const double* __restrict__ C, int K, int Kpad, int d, int xf64,
                                  float* __restrict__ CT32, float* __restrict__ cconst,
                                  float* __restrict__ chunkc, int metric) {
    // one wave per centroid: CT32 [d][Kpad], cconst [Kpad], chunkc {ec, eb}[Kpad/64]
    // (chunk maxima by atomicMax on the bits of positive floats; zeroed first).
    // cosine: CT32 holds the normalised row (score -x.c^), cconst 0, or +inf for
    // a zero / extreme-norm centroid (rows then evaluate every centroid exactly)
    const int c = blockIdx.x, lane = threadIdx.x;
    double scale = 1.0;
    if (metric == 1) {
        double q = 0.0;
        for (int j = lane; j < d; j += 64) {
            const double v = c < K ? C[(size_t)c * d + j] : 0.0;
            q = fma(v, v, q);
        }
        for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off);
        scale = (q >= 1e-200 && q <= 1e200) ? 1.0 / sqrt(q) : 0.0;
        if (c < K && scale == 0.0) {
            for (int j = lane; j < d; j += 64) CT32[(size_t)j * Kpad + c] = 0.f;
            if (lane == 0) cconst[c] = __builtin_inff();
            return;
        }
    }
    double sq = 0.0;
    for (int j = lane; j < d; j += 64) {
        const double v = c < K ? C[(size_t)c * d + j] * scale : 0.0;
        sq = fma(v, v, sq);
        CT32[(size_t)j * Kpad + c] = (float)v;
    }
    for (int off = 32; off >= 1; off >>= 1) sq += __shfl_xor(sq, off);
    if (lane != 0) return;
    if (c >= K) { cconst[c] = __builtin_inff(); return; }
    unsigned int* chunk = reinterpret_cast<unsigned int*>(chunkc + 2 * (c / 64));
    if (metric == 1) {
        // |s~ - x.c^| <= (d + 2) 2^-24 |x| (f32 FMA chain, c^'s f32 rounding), and
        // the reference's q = x.c / (|x||c|) sits within 2^-40 |x| of x.c^ / |x| . |x|
        cconst[c] = 0.f;
        const double ec = ((d + 2.0) * 0x1p-24 * (1.0 + 0x1p-10) + 0x1p-40 + (xf64 ? 0x1p-23 : 0.0)) * (1.0 + 0x1p-18);
        atomicMax(chunk, __float_as_uint((float)(ec * (1.0 + 0x1p-20))));
        atomicMax(chunk + 1, __float_as_uint(1e-30f));
        return;
    }
    const double up = 1.0 + 0x1p-18;
    const double nc = sqrt(sq) * (1.0 + 0x1p-30);
    cconst[c] = (float)sq;
    // fp64 rows are scored from their f32 roundings (as centroid_prep_kernel)
    const double ec = 0x1p-24 * (2.0 * d + 12.0 + (xf64 ? 2.0 : 0.0)) * nc * up;
    const double eb = (0x1p-24 * 5.0 * sq + 0x1p-40 * sq + (xf64 ? 0x1p-140 * nc : 0.0)) * up + 1e-30;
    atomicMax(chunk, __float_as_uint((float)(ec * (1.0 + 0x1p-20))));
    atomicMax(chunk + 1, __float_as_uint((float)(eb * (1.0 + 0x1p-20))));
}

// Phase 1: acc[r][i] = x_r . CT32 column lane + 64 i over NCH chunks of 64
// centroids. Chunks past Kpad read chunk 0 (their scores are never used): the
// loads carry no branch, so the unrolled iterations' loads issue together.
template <int UNROLL, int R, int NCH, typename TX>
__device__ inline void score_chunks(const float* __restrict__ CT32, int Kpad, int d, const TX (*xs)[XB_DMAX],
                                    float (&acc)[R][NCH]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int i = 0; i < NCH; i++) acc[r][i] = 0.f;
    int coff[NCH];
#pragma unroll
    for (int i = 0; i < NCH; i++) coff[i] = (64 * i < Kpad ? 64 * i : 0) + lane;
#pragma unroll UNROLL
    for (int j = 0; j < d; j++) {
        float cv[NCH];
#pragma unroll
        for (int i = 0; i < NCH; i++) cv[i] = CT32[(size_t)j * Kpad + coff[i]];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float xj = (float)xs[r][j];
#pragma unroll
            for (int i = 0; i < NCH; i++) acc[r][i] = fmaf(xj, cv[i], acc[r][i]);
        }
    }
}

// One row's bound, U = min (s~ + e) and candidate ballots cm (wave-uniform),
// ncand their count; false: no candidate, or a score that is not finite.
template <int MET, typename TX, int NCH>
__device__ inline bool row_candidates(float xn2p, const float (&acc)[NCH], const float* __restrict__ cconst,
                                      const float* __restrict__ chunkc, int K, unsigned long long (&cm)[NCH],
                                      int& ncand) {
    const int lane = threadIdx.x & 63;
    // |x|^2 in fp64 over the lanes' f32 partials, rounded up (as the f32 path)
    double xn2 = (double)xn2p;
    for (int off = 32; off >= 1; off >>= 1) xn2 += __shfl_xor(xn2, off);
    xn2 = xn2 * (sizeof(TX) == 4 ? 1.0 + 0x1p-20 : 1.0 + 0x1p-19) + (sizeof(TX) == 4 ? 0.0 : 0x1p-280);
    const float nx = (float)(sqrt(xn2) * (1.0 + 0x1p-30));
    const float ex = (float)(0x1p-40 * xn2 * (1.0 + 0x1p-18) + 1e-30);
    float lo[NCH];
    float U = __builtin_inff();
    bool finite = nx <= 3.0e38f;
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        const int c = lane + 64 * i;
        lo[i] = __builtin_inff();
        if (c < K) {
            const float E = fmaf(nx, chunkc[2 * i], chunkc[2 * i + 1] + ex);
            const float sc = MET == 1 ? cconst[c] - acc[i] : fmaf(-2.f, acc[i], cconst[c]);
            lo[i] = sc - E;
            const float hi = sc + E;
            finite = finite && (hi - lo[i]) <= 3.0e38f;   // false for inf / nan
            U = fminf(U, hi);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) U = fminf(U, __shfl_xor(U, off));
    ncand = 0;
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        cm[i] = __ballot(lo[i] <= U);
        ncand += __popcll(cm[i]);
    }
    return __all(finite) && ncand >= 1;
}

// The whole wave decides one row: lane k takes the k-th of its (at most 64)
// candidates, or, prune false, the lanes share every centroid.
template <int MET, typename TX, int NCH>
__device__ inline void wave_decide(const TX* xr, const double* __restrict__ C, int d, int K, bool prune,
                                   const unsigned long long (&cm)[NCH], bool exact_dist, int64_t row,
                                   int32_t* __restrict__ assign, double* __restrict__ dist) {
    double best = 0.0;
    int bi = -1;
    if (prune) {
        const int c = kth_candidate(cm, threadIdx.x & 63);
        if constexpr (MET == 0) {
            pruned_pick_euclid<64>(xr, C, d, c, exact_dist, best, bi);
        } else if (c >= 0) {
            best = pruned_dist<MET>(xr, C + (size_t)c * d, d);
            bi = c;
        }
    } else if (!(MET == 1 && cosine_nonfinite_row(xr, d, best, bi))) {
        every_centroid(K, [&](int c) { return pruned_dist<MET>(xr, C + (size_t)c * d, d); }, best, bi);
    }
    wave_store(best, bi, row, assign, dist);
}

// The wide form's walk over a segmented list (one segment per fused block): the
// groups of every segment in one flat index space, so the waves share the work
// whatever the segments' sizes (per-segment waves left the pass waiting on the
// fullest segments). gpre[s]: the groups before segment s.
template <int R>
__device__ inline const int* seg_group_prefix(const int32_t* __restrict__ seg_counts, int nseg) {
    __shared__ int gpre[FUSED_MAX_SEGS + 1];
    for (int sg = threadIdx.x; sg < nseg; sg += blockDim.x) gpre[sg + 1] = (seg_counts[SEG_SLOTS * sg + SEG_ROWS] + R - 1) / R;
    __syncthreads();
    if (threadIdx.x == 0) {
        gpre[0] = 0;
        for (int sg = 0; sg < nseg; sg++) gpre[sg + 1] += gpre[sg];
    }
    __syncthreads();
    return gpre;
}

// WIDE false: NCH = 4 chunks (ceil64(K) <= 256), XP_R rows per wave, XP_SPLIT
// blocks per list segment, and the rows with at most RL candidates decided
// RL lanes each, all at once. WIDE true: NCH = 16, XPW_R rows per wave -- the
// centroid columns stream from L2 once per XPW_R rows -- the flat group space,
// and each row's candidates selected and evaluated in turn by the whole wave
// (per-row masks only: no [rows][chunks] mask array).
template <typename TX, int MET, bool WIDE>
__global__ __launch_bounds__(64 * XP_WAVES) void assign_pruned_kernel(
    const TX* __restrict__ X, int d, const double* __restrict__ C, const float* __restrict__ CT32,
    const float* __restrict__ cconst, const float* __restrict__ chunkc, int K, int Kpad,
    const int32_t* __restrict__ rows, const unsigned long long* __restrict__ row_count, int64_t max_rows,
    int32_t* __restrict__ assign, double* __restrict__ dist, const int32_t* __restrict__ seg_counts,
    int64_t seg_rows, int nseg, int exact_dist) {
    constexpr int NCH = WIDE ? 16 : 4, R = WIDE ? XPW_R : XP_R, UNROLL = WIDE ? 2 : 8;
    __shared__ TX xs[XP_WAVES][R][XB_DMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool flat_segs = WIDE && seg_counts;
    const ListWalk w = list_walk<XP_SPLIT, XP_WAVES>(rows, row_count, max_rows, flat_segs ? nullptr : seg_counts, seg_rows);
    int64_t ngroups = (w.total + R - 1) / R;
    const int* gpre = nullptr;
    if constexpr (WIDE) {
        if (flat_segs) {
            gpre = seg_group_prefix<R>(seg_counts, nseg);
            ngroups = gpre[nseg];
        }
    }
    for (int64_t g = w.g0; g < ngroups; g += w.gstride) {
        const int32_t* grows = w.rows;
        int64_t gbase = g * R, cnt = w.total;
        if constexpr (WIDE) {
            if (flat_segs) {
                int lo = 0, hi = nseg;                  // gpre[lo] <= g < gpre[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (gpre[mid] <= g) lo = mid; else hi = mid;
                }
                grows = rows + (int64_t)lo * seg_rows;
                gbase = (g - gpre[lo]) * R;
                cnt = seg_counts[SEG_SLOTS * lo + SEG_ROWS];
            }
        }
        int32_t myrow[R];
        const int nr = group_rows(grows, gbase, cnt, myrow);
        float xn2p[R];
        stage_rows(X, d, myrow, xs[wave], xn2p);
        float acc[R][NCH];
        score_chunks<UNROLL>(CT32, Kpad, d, xs[wave], acc);
        if constexpr (WIDE) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (r >= nr) break;                     // wave-uniform
                unsigned long long cm[NCH];
                int ncand;
                const bool ok = row_candidates<MET, TX>(xn2p[r], acc[r], cconst, chunkc, K, cm, ncand);
                wave_decide<MET>(xs[wave][r], C, d, K, ok && ncand <= 64, cm, exact_dist != 0, myrow[r], assign, dist);
            }
        } else {
            constexpr int RL = 64 / R;           // lanes per row in the packed phase
            unsigned long long cm[R][NCH];
            int ncand[R];
            bool pr[R];
#pragma unroll
            for (int r = 0; r < R; r++)
                pr[r] = row_candidates<MET, TX>(xn2p[r], acc[r], cconst, chunkc, K, cm[r], ncand[r]) && r < nr;
            // rows with <= RL candidates: lane RL r + k evaluates row r's k-th candidate
            {
                const int r = lane / RL, k = lane % RL;
                int c = -1;
#pragma unroll
                for (int rr = 0; rr < R; rr++)
                    if (rr == r && pr[rr] && ncand[rr] <= RL) c = kth_candidate(cm[rr], k);
                double best = 0.0;
                int bi = -1;
                if constexpr (MET == 0) {
                    pruned_pick_euclid<RL>(xs[wave][r], C, d, c, exact_dist != 0, best, bi);   // within the row's lanes
                } else {
                    if (c >= 0) {
                        best = pruned_dist<MET>(xs[wave][r], C + (size_t)c * d, d);
                        bi = c;
                    }
                    group_argmin<RL>(best, bi);
                }
                if (k == 0 && bi >= 0) {
                    assign[myrow[r]] = bi;
                    dist[myrow[r]] = best;
                }
            }
            // the other rows, one at a time with the whole wave
            for (int r = 0; r < nr; r++) {
                if (pr[r] && ncand[r] <= RL) continue;
                wave_decide<MET>(xs[wave][r], C, d, K, pr[r] && ncand[r] <= 64, cm[r], exact_dist != 0, myrow[r], assign, dist);
            }
        }
        wave_sync();
    }
}

// ---------------------------------------------------------------- launchers
int launch_exact_prep(hipStream_t s, const AssignJob& q, ExactForm form, void* ws) {
    const ExactWs w = exact_ws(form, q.d, q.K);
    char* base = static_cast<char*>(ws);
    if (form == ExactForm::batch) {
        const int64_t ne = (int64_t)q.d * w.Kpad;
        hipLaunchKernelGGL(transpose_centroids_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, q.C, q.K,
                           w.Kpad, q.d, reinterpret_cast<double*>(base + w.ct));
        return kstatus("transpose_centroids_kernel");
    }
    if (!exact_is_pruned(form)) return 0;
    if (q.d > XB_DMAX || q.K > XP_KMAX) {
        set_error("launch_exact_prep: unsupported shape");
        return -1;
    }
    if (hipMemsetAsync(base + w.chunk, 0, w.bytes - w.chunk, s) != hipSuccess) return kstatus("exact prep");
    hipLaunchKernelGGL(exact_prep_kernel, dim3((unsigned)w.Kpad), dim3(64), 0, s, q.C, q.K, w.Kpad, q.d, q.X.f64 ? 1 : 0,
                       reinterpret_cast<float*>(base + w.ct), reinterpret_cast<float*>(base + w.cconst),
                       reinterpret_cast<float*>(base + w.chunk), q.metric == 0 ? 0 : 1);
    return kstatus("exact_prep_kernel");
}

int launch_exact_pass(hipStream_t s, const AssignJob& q, const RowList& l, ExactForm form, const void* ws,
                      bool exact_dist, const double* xn2, const double* nbv) {
    if (l.bound <= 0) return 0;
    const int32_t* seg_counts = l.seg_counts();
    if ((form != ExactForm::every && (q.d > XB_DMAX || !l.p)) || (exact_is_pruned(form) && q.K > XP_KMAX) ||
        l.nseg > FUSED_MAX_SEGS) {
        set_error("launch_exact_pass: unsupported shape");
        return -1;
    }
    const ExactWs w = exact_ws(form, q.d, q.K);
    const char* base = static_cast<const char*>(ws);
    const dim3 grid((unsigned)exact_blocks(form, l.nseg, l.bound, l.p != nullptr));
    const int metric = q.metric == 0 ? 0 : 1;   // 1: cosine
    with_rows(q.X, [&](auto* X) {
        using TX = std::remove_cv_t<std::remove_pointer_t<decltype(X)>>;
        const auto pruned = [&](auto met, auto wide) {
            hipLaunchKernelGGL((assign_pruned_kernel<TX, decltype(met)::value, decltype(wide)::value>), grid, dim3(64 * XP_WAVES), 0, s, X, q.d,
                               q.C, reinterpret_cast<const float*>(base + w.ct),
                               reinterpret_cast<const float*>(base + w.cconst),
                               reinterpret_cast<const float*>(base + w.chunk), q.K, w.Kpad, l.p, l.count, l.bound,
                               q.assign, q.dist, seg_counts, l.seg_rows, l.nseg, exact_dist ? 1 : 0);
        };
        using Euclid = std::integral_constant<int, 0>;
        using Cosine = std::integral_constant<int, 1>;
        switch (form) {
            case ExactForm::every:
                hipLaunchKernelGGL(assign_exact_kernel<TX>, grid, dim3(64 * XE_WAVES), 0, s, X, q.d, q.C, q.K, metric,
                                   l.p, l.count, l.bound, q.assign, q.dist, seg_counts, l.seg_rows, xn2, nbv);
                break;
            case ExactForm::batch:
                hipLaunchKernelGGL(assign_exact_batch_kernel<TX>, grid, dim3(64 * XB_WAVES), 0, s, X, q.d,
                                   reinterpret_cast<const double*>(base + w.ct), q.K, w.Kpad, l.p, l.count, l.bound,
                                   q.assign, q.dist, seg_counts, l.seg_rows);
                break;
            case ExactForm::pruned:
                if (metric) pruned(Cosine{}, std::false_type{}); else pruned(Euclid{}, std::false_type{});
                break;
            case ExactForm::pruned_wide:
                if (metric) pruned(Cosine{}, std::true_type{}); else pruned(Euclid{}, std::true_type{});
                break;
        }
    });
    return kstatus("exact_pass.hip");
}

}  // namespace lshkm
