// assign.hip — Lloyd's nearest-centroid assignment on gfx950.
//
// Replaces lloyds_assignment (lib/clustering_phases/assignment.hpp:54-80) with
// CustVector::euclideanDistance (lib/data_structures/cust_vector.hpp:124-136)
// and cosineDistance (:139-155).
//
// Fast path (euclidean): a block owns 128 points (4 waves x 32). Each wave keeps
// its 32 points in registers as the B operand of v_mfma_f32_32x32x2_f32 (lane
// half h holds dims [h*DP/2, (h+1)*DP/2) of point lane&31), centroids stream
// through LDS in chunks of 64 as the A operand, and the accumulator tile
// D[centroid][point] comes out with the point on the lane, so the per-point
// reduction over centroids is register-local. The score is
// s_c = ||c||^2 - 2 x.c; the MFMA result is an f32 FMA chain, so
//   |s~_c - s_c| <= e_c = 2^-24 ((2DP+12) |x||c| + 5 ||c||^2) + 2^-40 (|x|^2+||c||^2)
// covers the chain, the fp32 rounding of c, and the epilogue roundings; the
// 2^-40 term also covers the reference's sequential-fp64 rounding and keeps
// sqrt'ed ties apart. A point is certified when exactly one centroid has
// s~_c - e_c <= min_c (s~_c + e_c); its distance is then recomputed in exact
// reference order (fp64, no FMA contraction: sum_j (x_j - c_j)^2, j = 0..d-1,
// then sqrt). Uncertified points (ties, duplicate centroids, near-ties) go
// to the listed exact pass (exact_pass.hip), which evaluates centroids in
// reference order and keeps the first minimum (strict '<', assignment.hpp:66).
#include "common.h"
#include "kernels.h"
#include "exact.h"

namespace lshkm {

constexpr int AS_THREADS = 256;
constexpr int AS_PB = 128;   // points per block
constexpr int AS_CC = 64;    // centroids per LDS chunk

typedef float floatx16 __attribute__((ext_vector_type(16)));

int assign_dp(int d) {
    const int dps[] = {16, 32, 64, 128, 256};
    for (int dp : dps)
        if (d <= dp) return dp;
    return 0;
}

__global__ void centroid_prep_kernel(const double* __restrict__ C, int K, int Kpad, int d, int DP, int metric,
                                     int xf64, float* __restrict__ C32, float* __restrict__ cconst) {
    // One wave per 64-centroid chunk. cconst = cn2[Kpad] ++ {ecmax, ebmax}[Kpad/64]:
    // the bound coefficients are taken as the max over the chunk, so the MFMA
    // epilogue needs one per-lane bound per chunk instead of per centroid.
    // Cosine (metric 1): cn2[c] = f32(1 / |c|) and the score is -(x.c)/|c|
    // (argmin = the reference's argmin of 1 - cos): |s~ - s| <= (DP + 4) 2^-24 |x|
    // (the f32 chain, c's f32 rounding, 1/|c| and the product's rounding), plus
    // 2^-40 |x| over the reference's last-bit roundings of 1 - ip / denom; a zero
    // centroid (and padding) gets NaN: never taken, never lowers the bound min.
    // fp64 rows (xf64) reach the MFMA rounded to f32: |x_j - f32(x_j)| <= 2^-24 |x_j|
    // + 2^-150, i.e. 2 2^-24 |x||c| more on the euclidean score (2^-24 |x| on the
    // cosine one) plus 2^-150 |c|_1 <= 2^-146 |c| (flushed tiny entries).
    const int c = blockIdx.x * 64 + threadIdx.x;
    const double xw = xf64 ? 2.0 : 0.0;
    float* cn2 = cconst;
    float* chunk = cconst + Kpad + 2 * blockIdx.x;
    double ec = 0.0, eb = 0.0;
    if (c >= K) {
        for (int j = 0; j < DP; j++) C32[(size_t)c * DP + j] = 0.f;
        cn2[c] = metric ? __builtin_nanf("") : __builtin_inff();
    } else {
        double s = 0.0;
        for (int j = 0; j < d; j++) {
            const double v = C[(size_t)c * d + j];
            s = fma(v, v, s);
            C32[(size_t)c * DP + j] = (float)v;
        }
        for (int j = d; j < DP; j++) C32[(size_t)c * DP + j] = 0.f;
        const double up = 1.0 + 0x1p-18;
        const double nc = sqrt(s) * (1.0 + 0x1p-30);
        if (metric == 0) {
            // |c| >= 2^50 (or non-finite) may overflow the f32 chain: no
            // certificate in this call (flag after the chunk bounds)
            cn2[c] = s < 0x1p100 ? (float)s : __builtin_inff();
            if (!(s < 0x1p100)) atomicOr(reinterpret_cast<unsigned int*>(cconst + Kpad + Kpad / 32), 1u);
            ec = 0x1p-24 * (2.0 * DP + 12.0 + xw) * nc * up;
            eb = (0x1p-24 * 5.0 * s + 0x1p-40 * s + (xf64 ? 0x1p-140 * nc : 0.0)) * up + 1e-30;
        } else {
            // 1e-20 <= |c|^2 < 1e30 keeps the f32 chain clear of overflow and of
            // flushed denormals beyond eb ((DP + 4) 2^-124 / |c| for products and
            // c's entries, 2^-116 for x's); outside it,
            // and for a zero centroid 0 (whose NaN the reference's sentinel takes
            // for every row, assignment.hpp:66), eb = inf leaves no certificate
            const bool ok = s >= 1e-20 && s < 1e30;
            const double rc = ok ? 1.0 / sqrt(s) : 0.0;
            cn2[c] = ok ? (float)rc : __builtin_nanf("");
            ec = (0x1p-24 * (DP + 20.0 + xw) + 0x1p-40) * up;
            eb = ok ? ((DP + 4.0) * 0x1p-124 * rc + 0x1p-116) * up
                    : (s == 0.0 && c > 0 ? 0.0 : __builtin_inf());
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        ec = fmax(ec, __shfl_xor(ec, off));
        eb = fmax(eb, __shfl_xor(eb, off));
    }
    if (threadIdx.x == 0) {
        chunk[0] = (float)(ec * (1.0 + 0x1p-20));
        chunk[1] = (float)(eb * (1.0 + 0x1p-20));
    }
}

int launch_centroid_prep(hipStream_t s, const double* C, int K, int Kpad, int d, int DP, int metric, bool xf64,
                         float* C32, float* cconst) {
    (void)hipMemsetAsync(cconst + Kpad + Kpad / 32, 0, 4, s);
    hipLaunchKernelGGL(centroid_prep_kernel, dim3((Kpad + 63) / 64), dim3(64), 0, s, C, K, Kpad, d, DP, metric,
                       xf64 ? 1 : 0, C32, cconst);
    return kstatus("assign.hip");
}

template <int DP, int MET, typename TX>
__global__ __launch_bounds__(AS_THREADS, 2) void assign_mfma_kernel(
    const TX* __restrict__ X, int64_t N, int d, const double* __restrict__ C, int Kpad,
    const float* __restrict__ C32, const float* __restrict__ cconst, int32_t* __restrict__ assign,
    double* __restrict__ dist, int32_t* __restrict__ ambig, unsigned long long* __restrict__ ambig_count) {
    constexpr int H = DP / 2;     // dims per lane half
    constexpr int DS = DP + 4;    // padded LDS row stride (floats): conflict-free ds_read_b128
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lds = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int64_t pbase = (int64_t)blockIdx.x * AS_PB + wave * 32;

    // ---- phase 0: this wave's 32 rows -> LDS -> registers (B operand)
    float* xs = lds + wave * 32 * DS;
    if (d == DP) {
        for (int e4 = lane; e4 < 32 * DP / 4; e4 += 64) {
            const int r = e4 / (DP / 4), j = (e4 % (DP / 4)) * 4;
            const int64_t row = pbase + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (sizeof(TX) == 4) {
                if (row < N) v = *reinterpret_cast<const float4*>(X + row * DP + j);
            } else if (row < N) {
                const double2 a = *reinterpret_cast<const double2*>(X + row * DP + j);
                const double2 b = *reinterpret_cast<const double2*>(X + row * DP + j + 2);
                v = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
            }
            *reinterpret_cast<float4*>(xs + r * DS + j) = v;
        }
    } else if (sizeof(TX) == 8 && (d & 1) == 0) {
        // fp64 rows of even d (the recommender's user vectors, d = number of coins):
        // 16-B loads, a row per 64-lane pass (was one 8-B load per element)
        for (int e2 = lane; e2 < 32 * DP / 2; e2 += 64) {
            const int r = e2 / (DP / 2), j = (e2 % (DP / 2)) * 2;
            const int64_t row = pbase + r;
            float2 v = make_float2(0.f, 0.f);
            if (row < N && j < d) {
                const double2 a = *reinterpret_cast<const double2*>(X + row * d + j);
                v = make_float2((float)a.x, (float)a.y);
            }
            *reinterpret_cast<float2*>(xs + r * DS + j) = v;
        }
    } else if (sizeof(TX) == 4 && (d & 3) == 0) {
        for (int e4 = lane; e4 < 32 * DP / 4; e4 += 64) {
            const int r = e4 / (DP / 4), j = (e4 % (DP / 4)) * 4;
            const int64_t row = pbase + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < N && j < d) v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(X) + row * d + j);
            *reinterpret_cast<float4*>(xs + r * DS + j) = v;
        }
    } else {
        for (int e = lane; e < 32 * DP; e += 64) {
            const int r = e / DP, j = e % DP;
            const int64_t row = pbase + r;
            xs[r * DS + j] = (row < N && j < d) ? (float)X[row * d + j] : 0.f;
        }
    }
    __syncthreads();
    float b[H];
#pragma unroll
    for (int s = 0; s < H; s += 4) {
        const float4 v = *reinterpret_cast<const float4*>(xs + col * DS + h * H + s);
        b[s] = v.x; b[s + 1] = v.y; b[s + 2] = v.z; b[s + 3] = v.w;
    }
    double xn2 = 0.0;
#pragma unroll
    for (int s = 0; s < H; s++) xn2 = fma((double)b[s], (double)b[s], xn2);
    xn2 += __shfl_xor(xn2, 32);
    if (sizeof(TX) == 8) xn2 = xn2 * (1.0 + 0x1p-21) + 0x1p-280;   // |x|^2 from the f32-rounded row: still an upper bound
    const float nx = (float)(sqrt(xn2) * (1.0 + 0x1p-30));
    // cosine: |x| >= 1e18 may overflow the f32 products (|c| < 1e15 is checked
    // in the prep): no certificate, the row goes to the exact pass
    // |x| >= 2^50 (euclidean) / 1e18 (cosine) may overflow the f32 products: no
    // certificate, the row goes to the exact pass (false for inf / nan too)
    const float ex = MET == 0 ? (xn2 < 0x1p100 ? (float)(0x1p-40 * xn2 * (1.0 + 0x1p-18) + 1e-30) : __builtin_inff())
                              : (xn2 < 1e36 ? 0.f : __builtin_inff());
    __syncthreads();   // LDS now reused for centroid chunks

    float L1 = __builtin_inff(), L2 = __builtin_inff(), U = __builtin_inff();
    int i1 = 0;
    float* cs = lds;                 // [64][DS]
    float* cc = lds + AS_CC * DS;    // [64] cn2 of the chunk
    const float* chunkc = cconst + Kpad;
    for (int c0 = 0; c0 < Kpad; c0 += AS_CC) {
        for (int e4 = threadIdx.x; e4 < AS_CC * DP / 4; e4 += AS_THREADS) {
            const int r = e4 / (DP / 4), j = (e4 % (DP / 4)) * 4;
            *reinterpret_cast<float4*>(cs + r * DS + j) =
                *reinterpret_cast<const float4*>(C32 + (size_t)(c0 + r) * DP + j);
        }
        if (threadIdx.x < AS_CC) cc[threadIdx.x] = cconst[c0 + threadIdx.x];
        const float E = fmaf(nx, chunkc[2 * (c0 / AS_CC)], chunkc[2 * (c0 / AS_CC) + 1] + ex);
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < AS_CC / 32; t++) {
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
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int cb = t * 32 + 8 * g + 4 * h;   // D rows of registers 4g..4g+3
                const float4 cn = *reinterpret_cast<const float4*>(cc + cb);
                const float cnv[4] = {cn.x, cn.y, cn.z, cn.w};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float sc = MET == 0 ? fmaf(-2.f, acc[4 * g + q], cnv[q]) : -acc[4 * g + q] * cnv[q];
                    const float lo = sc - E, hi = sc + E;
                    if (lo < L1) { L2 = L1; L1 = lo; i1 = c0 + cb + q; }
                    else if (lo < L2) L2 = lo;
                    U = fminf(U, hi);
                }
            }
        }
        __syncthreads();
    }

    // ---- merge the two lane halves that share a point
    const float oL1 = __shfl_xor(L1, 32), oL2 = __shfl_xor(L2, 32), oU = __shfl_xor(U, 32);
    const int oi1 = __shfl_xor(i1, 32);
    float nL2; int ni1;
    if (oL1 < L1 || (oL1 == L1 && oi1 < i1)) { ni1 = oi1; nL2 = fminf(L1, oL2); }
    else { ni1 = i1; nL2 = fminf(oL1, L2); }
    U = fminf(U, oU);
    const bool cbad = __float_as_uint(cconst[Kpad + Kpad / 32]) != 0u;   // centroid out of the f32 range
    const bool cert = !cbad && nL2 > U;
    const int64_t row = pbase + col;
    const bool valid = row < N;

    // ---- exact-order distance of the certified winner: lanes h=0 sum dims
    // [0,H), hand the partial to lane h=1, which sums [H,2H) (j ascending).
    if (MET == 1) {
        // cosine (metric.hpp cosine distance): exact.h's certified fast form,
        // soft-x87 for the rows it cannot certify
        // soft-x87 for the rows it cannot certify, listed (after the ambiguous
        // rows' half of the list) for cos_fix_kernel: inline, one failing lane
        // would make its whole wave pay the soft chain
        bool fix = false;
        if (h == 1 && valid) {
            if (cert) {
                assign[row] = ni1;
                double v;
                if (cosine_fast(X + row * d, C + (size_t)ni1 * d, d, v)) dist[row] = v;
                else fix = true;
            } else {
                const unsigned long long slot = atomicAdd(ambig_count, 1ull);
                ambig[slot] = (int32_t)row;
            }
        }
        seg_append(fix, (int32_t)row, ambig_count + 1, ambig + N, lane);
        return;
    }
    double accd = 0.0;
    const TX* xrow = X + (valid ? row : 0) * d;
    if (h == 0 && cert && valid) {
        const double* crow = C + (size_t)ni1 * d;
#pragma unroll
        for (int s = 0; s < H; s++)
            if (s < d) {
                const double xv = sizeof(TX) == 4 ? (double)b[s] : (double)xrow[s];
                const double df = __dsub_rn(xv, crow[s]);
                accd = __dadd_rn(accd, gp_sq(df));
            }
    }
    const double part = __shfl_xor(accd, 32);
    if (h == 1 && valid) {
        if (cert) {
            double a2 = part;
            const double* crow = C + (size_t)ni1 * d;
#pragma unroll
            for (int s = 0; s < H; s++)
                if (H + s < d) {
                    const double xv = sizeof(TX) == 4 ? (double)b[s] : (double)xrow[H + s];
                    const double df = __dsub_rn(xv, crow[H + s]);
                    a2 = __dadd_rn(a2, gp_sq(df));
                }
            assign[row] = ni1;
            dist[row] = sqrt(a2);
        } else {
            const unsigned long long slot = atomicAdd(ambig_count, 1ull);
            ambig[slot] = (int32_t)row;
        }
    }
}

template <typename TX>
static int assign_mfma_tx(hipStream_t s, const TX* X, int64_t N, int d, int DP, const double* C, int Kpad, int metric,
                          const float* C32, const float* cconst, int32_t* assign, double* dist, int32_t* ambig,
                          unsigned long long* ambig_count) {
    const dim3 grid((unsigned)((N + AS_PB - 1) / AS_PB)), block(AS_THREADS);
    const size_t lds = (size_t)4 * 32 * (DP + 4) * 4;   // >= chunk (64*(DP+4) + 192) floats
    switch (DP * 2 + (metric ? 1 : 0)) {
#define AS_CASE(V) \
        case 2 * V: hipLaunchKernelGGL((assign_mfma_kernel<V, 0, TX>), grid, block, lds, s, X, N, d, C, Kpad, C32, cconst, assign, dist, ambig, ambig_count); break; \
        case 2 * V + 1: hipLaunchKernelGGL((assign_mfma_kernel<V, 1, TX>), grid, block, lds, s, X, N, d, C, Kpad, C32, cconst, assign, dist, ambig, ambig_count); break;
        AS_CASE(16) AS_CASE(32) AS_CASE(64) AS_CASE(128) AS_CASE(256)
#undef AS_CASE
        default: return -4;
    }
    return kstatus("assign.hip");
}

int launch_assign_mfma(hipStream_t s, Pts X, int64_t N, int d, int DP, const double* C, int K, int Kpad, int metric,
                       const float* C32, const float* cconst, int32_t* assign, double* dist, int32_t* ambig,
                       unsigned long long* ambig_count) {
    (void)K;
    if (N <= 0) return 0;
    return X.f64 ? assign_mfma_tx(s, X.d(), N, d, DP, C, Kpad, metric, C32, cconst, assign, dist, ambig, ambig_count)
                 : assign_mfma_tx(s, X.f(), N, d, DP, C, Kpad, metric, C32, cconst, assign, dist, ambig, ambig_count);
}

// Certified cosine winners whose distance IpAcc could not certify: one lane
// per listed row, the soft-x87 chain (exact.h exact_cosine_x87).
template <typename TX>
__global__ __launch_bounds__(256) void cos_fix_kernel(const TX* __restrict__ X, int d, const double* __restrict__ C,
                                                      const int32_t* __restrict__ rows,
                                                      const unsigned long long* __restrict__ count,
                                                      const int32_t* __restrict__ assign, double* __restrict__ dist) {
    const int64_t n = (int64_t)*count;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t row = rows[i];
        dist[row] = exact_cosine_x87(X + row * d, C + (size_t)assign[row] * d, d);
    }
}

int launch_cos_fix(hipStream_t s, Pts X, int64_t N, int d, const double* C, const int32_t* rows,
                   const unsigned long long* count, const int32_t* assign, double* dist) {
    if (N <= 0) return 0;
    const dim3 grid((unsigned)std::min<int64_t>((N + 255) / 256, 2048));
    if (X.f64) hipLaunchKernelGGL(cos_fix_kernel<double>, grid, dim3(256), 0, s, X.d(), d, C, rows, count, assign, dist);
    else hipLaunchKernelGGL(cos_fix_kernel<float>, grid, dim3(256), 0, s, X.f(), d, C, rows, count, assign, dist);
    return kstatus("assign.hip");
}

// Centroid override (assignment.hpp:77-78): in c order, so the last centroid
// that points at a row wins.
__global__ void assign_override_kernel(const int32_t* __restrict__ src, int K, int64_t N,
                                       int32_t* __restrict__ assign, double* __restrict__ dist) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K) return;
    const int32_t r = src[c];
    if (r < 0 || r >= N) return;
    for (int c2 = c + 1; c2 < K; c2++)      // a later centroid on the same row wins
        if (src[c2] == r) return;
    assign[r] = c;
    dist[r] = 0.0;
}

// Same, one block with the K source rows in LDS (K <= OV_LDS_MAX): thread c
// scans the later entries 4 at a time (ds_read_b128, 4 independent reads in
// flight) instead of K^2/2 dependent global loads.
constexpr int OV_LDS_MAX = 8192;
// ls: the block's (K + 15 & ~15) + 16 words
__device__ inline void override_lds(const int32_t* __restrict__ src, int K, int64_t N, int32_t* __restrict__ assign,
                                    double* __restrict__ dist, int32_t* ls) {
    const int Kp = (K + 15) & ~15;
    for (int c = threadIdx.x; c < Kp + 16; c += blockDim.x) ls[c] = c < K ? src[c] : -1;
    __syncthreads();
    for (int c = threadIdx.x; c < K; c += blockDim.x) {
        const int32_t r = ls[c];
        if (r < 0 || r >= N) continue;
        bool later = false;
        for (int b = (c + 1) & ~15; b < Kp && !later; b += 16) {
            const int4 v0 = *reinterpret_cast<const int4*>(ls + b);
            const int4 v1 = *reinterpret_cast<const int4*>(ls + b + 4);
            const int4 v2 = *reinterpret_cast<const int4*>(ls + b + 8);
            const int4 v3 = *reinterpret_cast<const int4*>(ls + b + 12);
            const int w[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w,
                               v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
#pragma unroll
            for (int t = 0; t < 16; t++) later |= b + t > c && w[t] == r;
        }
        if (!later) {                     // a later centroid on the same row wins
            assign[r] = c;
            dist[r] = 0.0;
        }
    }
}
__global__ __launch_bounds__(1024) void assign_override_lds_kernel(const int32_t* __restrict__ src, int K, int64_t N,
                                                                  int32_t* __restrict__ assign,
                                                                  double* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) int32_t ls[OV_LDS_MAX + 16];
    override_lds(src, K, N, assign, dist, ls);
}

int launch_assign_override(hipStream_t s, const int32_t* src_rows, int K, int64_t N, int32_t* assign,
                           double* dist) {
    if (K <= OV_LDS_MAX)
        hipLaunchKernelGGL(assign_override_lds_kernel, dim3(1), dim3(1024), 0, s, src_rows, K, N, assign, dist);
    else
        hipLaunchKernelGGL(assign_override_kernel, dim3((K + 255) / 256), dim3(256), 0, s, src_rows, K, N, assign,
                           dist);
    return kstatus("assign.hip");
}

__global__ void add_counter_kernel(unsigned long long* dst, const unsigned long long* src) {
    if (threadIdx.x == 0) *dst += *src;
}

int launch_add_counter(hipStream_t s, unsigned long long* dst, const unsigned long long* src) {
    hipLaunchKernelGGL(add_counter_kernel, dim3(1), dim3(1), 0, s, dst, src);
    return kstatus("assign.hip");
}

// stats[dst_idx[i]] += src[i] for i < n (n <= 8): the per-call statistics in one launch
struct CounterAdds {
    int n;
    int dst[8];
    const unsigned long long* src[8];
};
__global__ void add_counters_kernel(unsigned long long* stats, CounterAdds c) {
    if ((int)threadIdx.x < c.n) atomicAdd(stats + c.dst[threadIdx.x], *c.src[threadIdx.x]);
}

int launch_add_counters(hipStream_t s, unsigned long long* stats, int n, const int* dst_idx,
                        const unsigned long long* const* src) {
    if (n <= 0) return 0;
    if (n > 8) {
        set_error("launch_add_counters: at most 8 counters");
        return -1;
    }
    CounterAdds c;
    c.n = n;
    for (int i = 0; i < n; i++) { c.dst[i] = dst_idx[i]; c.src[i] = src[i]; }
    hipLaunchKernelGGL(add_counters_kernel, dim3(1), dim3(64), 0, s, stats, c);
    return kstatus("assign.hip");
}

// The fused assignment's epilogue, one small block (it is placed beside the
// hash fix-up's blocks as soon as one of them ends): the call's counters added
// into the context's, the counters and the centroid prep's bound words then
// zeroed for the next call (fused.hip: a clean workspace needs no clears), and
// the centroid override where the call has one (src != NULL, K <= OV_LDS_MAX).
// EPI_THREADS threads without an override or with few centroids; with more
// centroids as many as the override's own kernel, up to EPI_THREADS_MAX (its
// scan of the later entries is quadratic in K).
constexpr int EPI_THREADS = 256, EPI_THREADS_MAX = 1024;
__global__ __launch_bounds__(EPI_THREADS_MAX) void fused_epilogue_kernel(unsigned long long* stats, CounterAdds c,
                                                                     unsigned long long* cnt, int ncnt,
                                                                     unsigned int* cb, int ncb,
                                                                     const int32_t* __restrict__ src, int K, int64_t N,
                                                                     int32_t* __restrict__ assign,
                                                                     double* __restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) int32_t epi_ls[];
    if ((int)threadIdx.x < c.n) atomicAdd(stats + c.dst[threadIdx.x], *c.src[threadIdx.x]);
    __syncthreads();                      // every counter read before any is zeroed
    if ((int)threadIdx.x < ncnt) cnt[threadIdx.x] = 0ull;
    if ((int)threadIdx.x < ncb) cb[threadIdx.x] = 0u;
    if (src) override_lds(src, K, N, assign, dist, epi_ls);
}

int launch_fused_epilogue(hipStream_t s, unsigned long long* stats, int n, const int* dst_idx,
                          const unsigned long long* const* srcs, unsigned long long* cnt, int ncnt, unsigned int* cb,
                          int ncb, const int32_t* src_rows, int K, int64_t N, int32_t* assign, double* dist) {
    if (n > 8 || ncnt > EPI_THREADS || ncb > EPI_THREADS) {
        set_error("launch_fused_epilogue: at most 8 counters and 256 words to zero");
        return -1;
    }
    CounterAdds c;
    c.n = n;
    for (int i = 0; i < n; i++) { c.dst[i] = dst_idx[i]; c.src[i] = srcs[i]; }
    // more centroids than the LDS form holds: the override's global-memory
    // kernel after the epilogue (it touches assign / dist alone)
    const bool own_launch = src_rows && K > OV_LDS_MAX;
    const int32_t* src = own_launch ? nullptr : src_rows;
    const size_t lds = src ? ((size_t)((K + 15) & ~15) + 16) * 4 : 0;
    const int threads = src ? std::min(EPI_THREADS_MAX, std::max(EPI_THREADS, (K + 63) / 64 * 64)) : EPI_THREADS;
    hipLaunchKernelGGL(fused_epilogue_kernel, dim3(1), dim3(threads), lds, s, stats, c, cnt, ncnt, cb, ncb, src, K, N,
                       assign, dist);
    if (own_launch) {
        const int rc = kstatus("fused_epilogue_kernel");
        return rc ? rc : launch_assign_override(s, src_rows, K, N, assign, dist);
    }
    return kstatus("fused_epilogue_kernel");
}

}  // namespace lshkm
