// pam.hip — the PAM medoid update on gfx950.
//
// Replaces: pam_lloyds (lib/clustering_phases/update.hpp:89-142) over the
// clusters of separate_clusters_from_input (lib/utils.hpp:150-158).
//
//   dist_sum(p) = sum_{j in cluster} dist(x_p, x_j)  in member order, j = p
//                 included, from 0.0 by sequential fp64 adds
//   medoid      = min = -1; for p: if (min == -1 || dist_sum(p) < min) take p
//                 (strict <: the first of equal sums; the first member is taken
//                 whatever its sum, a NaN min is never replaced, a NaN sum
//                 never replaces a finite min)
// Every distance is the reference's exact one (exact.h, pairsum.h). The
// reference's distance cache (keyed "<id>to<id>", update.hpp:108-121) stores
// d(x_p, x_j) for the reverse pair; d is bitwise symmetric in both metrics
// (negated differences square alike, products and the two norms commute), so
// recomputing it gives the cached value for unique IDs.
//
// Two paths, the same answer bit for bit:
//   exact   every member's dist_sum by pairsum.h's chain (pam_exact_kernel),
//           then the selection in member order (pam_select_kernel).
//   screen  (euclidean) the members' Gram matrix tile by tile on the f32 MFMA:
//           d~ = sqrt(|p|^2 + |j|^2 - 2 p.j), S~(p) = sum_j d~, with a rigorous
//           bound E(p) on |S~(p) - dist_sum(p)| (pam_screen_kernel); only the
//           members with S~ - E <= min_p (S~ + E) can hold the minimum or tie
//           it, and only they go to the exact chain, in member order.
#include "common.h"
#include "exact.h"
#include "kernels.h"
#include "pairsum.h"
#include "tile.h"

namespace lshkm {

// ------------------------------------------------------------------ arguments
__global__ void pam_check_assign_kernel(const int32_t* __restrict__ assign, int64_t N, int K, int* __restrict__ bad) {
    bool b = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int a = assign[i];
        b |= a < 0 || a >= K;
    }
    if (b) atomicOr(bad, 1);
}

int launch_pam_check_assign(hipStream_t s, const int32_t* assign, int64_t N, int K, int* bad) {
    (void)hipMemsetAsync(bad, 0, 4, s);
    if (N > 0)
        hipLaunchKernelGGL(pam_check_assign_kernel, dim3(gsz(N, 256, 4096)), dim3(256), 0, s, assign, N, K, bad);
    return kstatus("pam_check_assign_kernel");
}

// ----------------------------------------------------------------- exact path
// One wave per two consecutive candidates (pairsum.h): one pass over the x_j
// when they share a cluster (euclidean, d % 4 == 0).
constexpr int PE_WAVES = 4;
constexpr int PAM_DMAX = 512;            // rows up to this many dims sit in LDS

template <typename TX, bool EXSQ>
__global__ __launch_bounds__(64 * PE_WAVES) void pam_exact_kernel(
    const TX* __restrict__ X, int d, int metric, const int32_t* __restrict__ rows, const int64_t* __restrict__ crow,
    const int32_t* __restrict__ assign, const int32_t* __restrict__ cand, const int64_t* __restrict__ m_dev, int64_t N,
    double* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) TX xs[PE_WAVES][2][PAM_DMAX];
    __shared__ double sqs[PE_WAVES][64 * 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* sq = sqs[wave];
    TX* xa = xs[wave][0];
    TX* xb = xs[wave][1];
    const int64_t M = m_dev ? *m_dev : N;
    const int64_t npair = (M + 1) / 2;
    for (int64_t q = (int64_t)blockIdx.x * PE_WAVES + wave; q < npair; q += (int64_t)gridDim.x * PE_WAVES) {
        const int64_t i = 2 * q;
        const bool has2 = i + 1 < M;
        const int64_t pa = cand ? cand[i] : i, pb = has2 ? (cand ? cand[i + 1] : i + 1) : pa;
        const int32_t ra = rows[pa], rb = rows[pb];
        const int ca = assign[ra], cb = assign[rb];
        __builtin_amdgcn_wave_barrier();                      // previous candidates' reads of xs are done
        for (int k = lane; k < d; k += 64) {
            xa[k] = X[(size_t)ra * d + k];
            xb[k] = X[(size_t)rb * d + k];
        }
        wave_sync();
        if (has2 && ca == cb && metric == 0 && (d & 3) == 0) {
            double s0, s1;
            sil_segment2<TX, EXSQ>(xa, xb, X, d, rows, crow[ca], crow[ca + 1], lane, s0, s1, sq);
            if (lane == 0) {
                sums[i] = x86_nan(s0);
                sums[i + 1] = x86_nan(s1);
            }
            continue;
        }
        for (int m = 0; m < (has2 ? 2 : 1); m++) {
            const int c = m ? cb : ca;
            const double sm = sil_segment<TX, EXSQ>(m ? xb : xa, X, d, metric, rows, crow[c], crow[c + 1], lane, sq);
            if (lane == 0) sums[i + m] = x86_nan(sm);
        }
    }
}

// d > PAM_DMAX: one thread per candidate, the same sums.
template <typename TX>
__global__ void pam_exact_thread_kernel(const TX* __restrict__ X, int d, int metric, const int32_t* __restrict__ rows,
                                        const int64_t* __restrict__ crow, const int32_t* __restrict__ assign,
                                        const int32_t* __restrict__ cand, const int64_t* __restrict__ m_dev, int64_t N,
                                        double* __restrict__ sums) {
    const int64_t M = m_dev ? *m_dev : N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = rows[cand ? cand[i] : i];
        const int c = assign[r];
        const TX* xi = X + (size_t)r * d;
        double a = 0.0;
        for (int64_t j = crow[c]; j < crow[c + 1]; j++)
            a = __dadd_rn(a, exact_dist(xi, X + (size_t)rows[j] * d, d, metric));
        sums[i] = x86_nan(a);
    }
}

template <typename TX>
static int pam_exact_tx(hipStream_t s, const TX* X, int d, int metric, const int32_t* rows, const int64_t* crow,
                        const int32_t* assign, const int32_t* cand, const int64_t* m_dev, int64_t N, double* sums,
                        bool exsq) {
    if (d > PAM_DMAX) {
        hipLaunchKernelGGL(pam_exact_thread_kernel<TX>, dim3(gsz(N, 256, 16384)), dim3(256), 0, s, X, d, metric, rows,
                           crow, assign, cand, m_dev, N, sums);
        return kstatus("pam_exact_thread_kernel");
    }
    const dim3 grid(gsz((N + 1) / 2, PE_WAVES, 16384)), block(64 * PE_WAVES);
    if (exsq)
        hipLaunchKernelGGL((pam_exact_kernel<TX, true>), grid, block, 0, s, X, d, metric, rows, crow, assign, cand, m_dev,
                           N, sums);
    else
        hipLaunchKernelGGL((pam_exact_kernel<TX, false>), grid, block, 0, s, X, d, metric, rows, crow, assign, cand,
                           m_dev, N, sums);
    return kstatus("pam_exact_kernel");
}

int launch_pam_exact(hipStream_t s, Pts X, int d, int metric, const int32_t* rows, const int64_t* crow,
                     const int32_t* assign, const int32_t* cand, const int64_t* m_dev, int64_t N, double* sums,
                     bool exsq) {
    if (N == 0) return 0;
    return X.f64 ? pam_exact_tx(s, X.d(), d, metric, rows, crow, assign, cand, m_dev, N, sums, exsq)
                 : pam_exact_tx(s, X.f(), d, metric, rows, crow, assign, cand, m_dev, N, sums, exsq);
}

// One wave per cluster: update.hpp:99-129's loop over the candidates' sums.
// Lane L scans candidates L, L + 64, ... (ascending), keeping its first
// minimum among the non-NaN sums; the lanes' (sum, index) pairs then reduce to
// the smallest sum at the lowest index -- the loop's result unless the first
// sum is NaN (then the first member stays).
__global__ __launch_bounds__(256) void pam_select_kernel(const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ cand,
                                                         const int64_t* __restrict__ coff, int K,
                                                         const double* __restrict__ sums, int32_t* __restrict__ med,
                                                         double* __restrict__ csum) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= K) return;
    const int64_t i0 = coff[c], i1 = coff[c + 1];
    if (i0 == i1) {
        if (lane == 0) { med[c] = -1; csum[c] = -1.0; }
        return;
    }
    const double first = sums[i0];
    double best = 0.0;
    int64_t bi = -1;
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        const double v = sums[i];
        if (v == v && (bi < 0 || v < best)) { best = v; bi = i; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(best, off);
        const int64_t oi = __shfl_xor(bi, off);
        if (oi >= 0 && (bi < 0 || ov < best || (ov == best && oi < bi))) { best = ov; bi = oi; }
    }
    if (first != first) { best = first; bi = i0; }
    if (lane == 0) {
        med[c] = rows[cand ? cand[bi] : bi];
        csum[c] = best;
    }
}

int launch_pam_select(hipStream_t s, const int32_t* rows, const int32_t* cand, const int64_t* coff, int K,
                      const double* sums, int32_t* med, double* csum) {
    hipLaunchKernelGGL(pam_select_kernel, dim3((K + 3) / 4), dim3(256), 0, s, rows, cand, coff, K, sums, med, csum);
    return kstatus("pam_select_kernel");
}

template <typename TX>
__global__ void pam_gather_kernel(const TX* __restrict__ X, int d, const int32_t* __restrict__ med,
                                  const double* __restrict__ C_old, double* __restrict__ C_new) {
    const int c = blockIdx.x;
    const int32_t r = med[c];
    for (int j = threadIdx.x; j < d; j += blockDim.x)
        C_new[(size_t)c * d + j] = r >= 0 ? (double)X[(size_t)r * d + j] : C_old[(size_t)c * d + j];
}

int launch_pam_gather(hipStream_t s, Pts X, int d, const int32_t* med, int K, const double* C_old, double* C_new) {
    if (X.f64) hipLaunchKernelGGL(pam_gather_kernel<double>, dim3(K), dim3(128), 0, s, X.d(), d, med, C_old, C_new);
    else hipLaunchKernelGGL(pam_gather_kernel<float>, dim3(K), dim3(128), 0, s, X.f(), d, med, C_old, C_new);
    return kstatus("pam_gather_kernel");
}

// --------------------------------------------------------------------- screen
// The bound. x^ = f32(x) (the MFMA operand), rho = |x - x^|_2, n2 = |x^|^2.
//   g~  the f32 MFMA chain of x^_m . x^_n over DP terms:
//         |g~ - x^_m . x^_n| <= (DP + 8) 2^-24 |x^_m| |x^_n|   (one rounding per
//         term, as assign.hip's score bound) + 2^-117 (1 + |x^_m| + |x^_n|)
//         (flushed subnormal operands, products and partial sums)
//   a   = n2_m + n2_n - 2 g~ in fp64 (n2: fp64 fma chains, 2^-44 relative):
//         |a - |x^_m - x^_n|^2| <= eps
//         eps = 2 (DP + 8) 2^-24 |x^_m| |x^_n| + 2^-43 (n2_m + n2_n)
//               + 2^-110 (1 + |x^_m| + |x^_n|)
//   t   = sqrtf(f32(max(a, 0))): |t - sqrt(max(a, 0))| <= 2^-22 t + 2^-63
//   | sqrt(max(a, 0)) - |x^_m - x^_n| | <= sqrt(eps), and <= eps / sqrt(a - eps)
//         <= 1.25 eps / t where a >= 4 eps. Near-duplicate rows (a ~ 0: the Gram
//         form cancels) take the sqrt(eps) branch, which needs no lower bound on a.
//   | |x^_m - x^_n| - |x_m - x_n| | <= rho_m + rho_n
//   the reference's own distance is within (d + 3) 2^-53 relative (+ 2^-530
//         where a square underflows) of |x_m - x_n|, its sequential sum within
//         n 2^-53 of the sum of its terms.
// Per pair e = [sqrt(eps) or 1.25 eps / t] + 2^-21 t + rho_m + rho_n + 2^-60;
// S~ and E of a member come in two parts, both independent of the order in
// which blocks run (no floating-point atomics): the column part accumulates in
// fp64 in the lane that owns the member, in walk order, the two half-waves
// added at the end; the row part arrives per tile as the f32 tree sum of 32
// terms (<= 2^-21 of the sum off, charged to E), truncated to fixed point (E's
// rounded up; one unit per piece, at most n / 32 pieces). pam_total closes the
// bound: E <- E (1 + 2^-9) + S~ (n + 64) 2^-50 + (n / 16 + 4) units for the f32
// roundings inside e, the fp64 accumulations, the reference's roundings and
// the truncations. Rows with |x| >= 2^50 or a
// non-finite value are outside what the bound assumes: their cluster is not
// screened (cbad).
constexpr int PS_THREADS = 256;
constexpr int PS_RB = 64;                // members staged in LDS per step

// One wave per member position: n2, rho, the cluster's range flag.
template <typename TX>
__global__ __launch_bounds__(256) void pam_prep_kernel(const TX* __restrict__ X, int d,
                                                       const int32_t* __restrict__ rows,
                                                       const int32_t* __restrict__ assign, int64_t N,
                                                       double* __restrict__ n2, float* __restrict__ rho,
                                                       int* __restrict__ cbad,
                                                       unsigned long long* __restrict__ cmax) {
    const int lane = threadIdx.x & 63;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < N; q += (int64_t)gridDim.x * 4) {
        const int32_t r = rows[q];
        double s = 0.0, rr = 0.0;
        bool bad = false;
        for (int j = lane; j < d; j += 64) {
            const double v = (double)X[(size_t)r * d + j];
            const float f = (float)v;
            const double fd = (double)f, dl = v - fd;
            bad |= !(fabs(v) < 0x1p60);
            s = fma(fd, fd, s);
            rr = fma(dl, dl, rr);
        }
        for (int off = 32; off >= 1; off >>= 1) {
            s += __shfl_xor(s, off);
            rr += __shfl_xor(rr, off);
        }
        bad = __any(bad) || !(s < 0x1p100);
        if (lane == 0) {
            n2[q] = s;
            rho[q] = bad ? 0.f : (float)(sqrt(rr) * (1.0 + 0x1p-20));
            if (bad) atomicOr(cbad + assign[r], 1);
            else atomicMax(cmax + assign[r], (unsigned long long)__double_as_longlong(s));   // s >= 0: bit order
        }
    }
}

int launch_pam_prep(hipStream_t s, Pts X, int d, const int32_t* rows, const int32_t* assign, int64_t N, double* n2,
                    float* rho, int* cbad, unsigned long long* cmax) {
    if (N == 0) return 0;
    const dim3 grid(gsz(N, 4, 8192));
    if (X.f64) hipLaunchKernelGGL(pam_prep_kernel<double>, grid, dim3(256), 0, s, X.d(), d, rows, assign, N, n2, rho, cbad, cmax);
    else hipLaunchKernelGGL(pam_prep_kernel<float>, grid, dim3(256), 0, s, X.f(), d, rows, assign, N, n2, rho, cbad, cmax);
    return kstatus("pam_prep_kernel");
}

// Fixed-point scale of a cluster's row parts (below): every t and e is below
// dmax = 2.5 max|x^| + 2^-40, and n dmax 2^k < 2^61, so a member's row part
// fits 64 bits whatever order its pieces arrive in.
__device__ inline double pam_scale(unsigned long long cmax_bits, int n) {
    const double dmax = 2.5 * sqrt(__longlong_as_double((long long)cmax_bits)) + 0x1p-40;
    const int k = 60 - ilogb(dmax * (double)n);
    return ldexp(1.0, min(max(k, -900), 900));
}

// v[i] summed over the 32 lanes of a half-wave for every i, by a fixed tree
// (reproducible): lane l returns register i = (l >> 1) & 15's total.
__device__ inline float half_reduce16(const float (&v)[16], int l5) {
    float a8[8], a4[4], a2[2];
    const bool u16 = l5 & 16, u8 = l5 & 8, u4 = l5 & 4, u2 = l5 & 2;
#pragma unroll
    for (int j = 0; j < 8; j++) a8[j] = (u16 ? v[j + 8] : v[j]) + __shfl_xor(u16 ? v[j] : v[j + 8], 16);
#pragma unroll
    for (int j = 0; j < 4; j++) a4[j] = (u8 ? a8[j + 4] : a8[j]) + __shfl_xor(u8 ? a8[j] : a8[j + 4], 8);
#pragma unroll
    for (int j = 0; j < 2; j++) a2[j] = (u4 ? a4[j + 2] : a4[j]) + __shfl_xor(u4 ? a4[j] : a4[j + 2], 4);
    const float a1 = (u2 ? a2[1] : a2[0]) + __shfl_xor(u2 ? a2[0] : a2[1], 2);
    return a1 + __shfl_xor(a1, 1);
}

// A block owns PAM_SCREEN_COLS members of one cluster (wave w: 32 of them, the
// MFMA's B operand, kept in registers) and walks other members PS_RB at a time
// (the A operand, staged in LDS for the four waves). The Gram matrix is
// symmetric, so of the cluster's G groups of PAM_SCREEN_COLS members block g
// walks only its own group and the next (G - 1) / 2 (cyclically: every block
// the same work, every unordered pair of groups seen by exactly one block). A
// tile of those serves both sides: its column sums go to the block's members
// (the lanes' fp64 S, E), its row sums to the walked members -- reduced over
// the half-wave by a fixed tree, then added as fixed-point integers (fix: S
// part, E part rounded up), which no order of arrival changes. The block's own
// group, and for even G the group opposite (which blocks g and g + G / 2 both
// see), give column sums only.
template <int DP, typename TX>
__global__ __launch_bounds__(PS_THREADS, 2) void pam_screen_kernel(
    const TX* __restrict__ X, int d, const int32_t* __restrict__ rows, const int64_t* __restrict__ crow,
    const int2* __restrict__ items, const double* __restrict__ n2, const float* __restrict__ rho,
    double* __restrict__ St, double* __restrict__ Et, const unsigned long long* __restrict__ cmax,
    unsigned long long* __restrict__ Sfix, unsigned long long* __restrict__ Efix) {
    constexpr int H = DP / 2;     // dims per lane half
    constexpr int DS = DP + 4;    // padded LDS row stride (floats): conflict-free ds_read_b128
    __shared__ __attribute__((aligned(16))) float cs[PS_RB * DS];
    __shared__ double rn2[PS_RB];
    __shared__ float rnm[PS_RB], rq[PS_RB], rrho[PS_RB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int2 it = items[blockIdx.x];
    const int64_t c0 = crow[it.x];
    const int n = (int)(crow[it.x + 1] - c0);
    const int jn = it.y + wave * 32 + col;          // this lane's member (both halves)
    const bool own = jn < n;

    float b[H];
    {
        const TX* xr = X + (size_t)rows[c0 + (own ? jn : 0)] * d;
#pragma unroll
        for (int s = 0; s < H; s++) b[s] = (own && h * H + s < d) ? (float)xr[h * H + s] : 0.f;
    }
    const double n2n = own ? n2[c0 + jn] : 0.0;
    const float up = 1.f + 0x1p-10f;
    const float nrmn = (float)(sqrt(n2n) * (1.0 + 0x1p-20));
    const float qn = (float)(n2n * 0x1p-43) * up + 0x1p-110f * (0.5f + nrmn);
    const float rhon = own ? rho[c0 + jn] : 0.f;
    const float ce = 2.f * (DP + 8) * 0x1p-24f * up * nrmn;

    const double scale = pam_scale(cmax[it.x], n);
    double S = 0.0, E = 0.0;
    // groups g, g + 1, ..., g + (G - 1) / 2 (mod G), and g + G / 2 for its own side only
    const int G = (n + PAM_SCREEN_COLS - 1) / PAM_SCREEN_COLS, g = it.y / PAM_SCREEN_COLS;
    const int half = (G - 1) / 2, nk = half + 1 + ((G & 1) == 0 ? 1 : 0);
    for (int step = 0; step < nk * (PAM_SCREEN_COLS / PS_RB); step++) {
        const int kk = step / (PAM_SCREEN_COLS / PS_RB);
        const int m0 = ((g + kk) % G) * PAM_SCREEN_COLS + (step % (PAM_SCREEN_COLS / PS_RB)) * PS_RB;
        if (m0 >= n) continue;                              // the last group's second half
        const bool both = kk >= 1 && kk <= half;            // this block alone sees these tiles
        if (sizeof(TX) == 4 && (d & 3) == 0) {
            for (int e4 = threadIdx.x; e4 < PS_RB * DP / 4; e4 += PS_THREADS) {
                const int r = e4 / (DP / 4), j = (e4 % (DP / 4)) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (m0 + r < n && j < d)
                    v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(X) +
                                                         (size_t)rows[c0 + m0 + r] * d + j);
                *reinterpret_cast<float4*>(cs + r * DS + j) = v;
            }
        } else {
            for (int e = threadIdx.x; e < PS_RB * DP; e += PS_THREADS) {
                const int r = e / DP, j = e % DP;
                cs[r * DS + j] = (m0 + r < n && j < d) ? (float)X[(size_t)rows[c0 + m0 + r] * d + j] : 0.f;
            }
        }
        if (threadIdx.x < PS_RB) {
            const int m = m0 + threadIdx.x;
            const double v = m < n ? n2[c0 + m] : 0.0;
            const float nm = (float)(sqrt(v) * (1.0 + 0x1p-20));
            rn2[threadIdx.x] = v;
            rnm[threadIdx.x] = nm;
            rq[threadIdx.x] = (float)(v * 0x1p-43) * up + 0x1p-110f * (0.5f + nm);
            rrho[threadIdx.x] = m < n ? rho[c0 + m] : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < PS_RB / 32; t++) {
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
            // register 4g + q holds member m = t * 32 + 8g + 4h + q of the step (D row)
            float tr[16], er[16];
#pragma unroll
            for (int g = 0; g < 4; g++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int ml = t * 32 + 8 * g + 4 * h + q;
                    const double a = fma(-2.0, (double)acc[4 * g + q], n2n + rn2[ml]);
                    const float am = fmaxf((float)a, 0.f);
                    const float tt = sqrtf(am);
                    const float eps = fmaf(ce, rnm[ml], qn + rq[ml]);
                    const float esq = am >= 4.f * eps ? 1.25f * eps / tt : sqrtf(eps) * up;
                    const float e = esq + tt * 0x1p-21f + rhon + rrho[ml] + 0x1p-60f;
                    const bool valid = m0 + ml < n;
                    S += valid ? (double)tt : 0.0;
                    E += valid ? (double)e : 0.0;
                    tr[4 * g + q] = valid && own ? tt : 0.f;
                    er[4 * g + q] = valid && own ? e : 0.f;
                }
            }
            if (both) {
                // the tree's f32 adds: 5 levels, <= 2^-21 of each total, into the E part
                const float rs = half_reduce16(tr, col), re = half_reduce16(er, col);
                const int i = col >> 1, m = m0 + t * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
                if ((col & 1) == 0 && m < n) {
                    atomicAdd(Sfix + c0 + m, (unsigned long long)((double)rs * scale));
                    atomicAdd(Efix + c0 + m, (unsigned long long)((double)(re * up + rs * 0x1p-20f) * scale) + 1ull);
                }
            }
        }
        __syncthreads();
    }
    // the two halves of a member's walk, always lower half first (pam_total adds
    // the row parts and the closing terms of the bound)
    const double So = __shfl_xor(S, 32), Eo = __shfl_xor(E, 32);
    if (own && h == 0) {
        St[c0 + jn] = S + So;
        Et[c0 + jn] = E + Eo;
    }
}

// A member's S~ and E: the column part plus the fixed-point row part, then the
// closing terms: the f32 roundings inside e, the fp64 accumulations and the
// reference's roundings, and one unit per row-part piece (at most n / 32) for
// the truncation to fixed point.
__device__ inline void pam_total(int64_t q, const double* __restrict__ St, const double* __restrict__ Et,
                                 const unsigned long long* __restrict__ Sfix,
                                 const unsigned long long* __restrict__ Efix, double unit, int n, double& S,
                                 double& E) {
    S = St[q] + (double)Sfix[q] * unit;
    E = (Et[q] + (double)Efix[q] * unit) * (1.0 + 0x1p-9) + S * ((double)n + 64.0) * 0x1p-50 +
        ((double)n / 16.0 + 4.0) * unit;
}

template <typename TX>
static int pam_screen_tx(hipStream_t s, const TX* X, int d, const int32_t* rows, const int64_t* crow, const int2* items,
                         int64_t nitems, const double* n2, const float* rho, double* St, double* Et,
                         const unsigned long long* cmax, unsigned long long* Sfix, unsigned long long* Efix) {
    const dim3 grid((unsigned)nitems), block(PS_THREADS);
    if (d <= 32)
        hipLaunchKernelGGL((pam_screen_kernel<32, TX>), grid, block, 0, s, X, d, rows, crow, items, n2, rho, St, Et, cmax,
                           Sfix, Efix);
    else
        hipLaunchKernelGGL((pam_screen_kernel<128, TX>), grid, block, 0, s, X, d, rows, crow, items, n2, rho, St, Et, cmax,
                           Sfix, Efix);
    return kstatus("pam_screen_kernel");
}

int launch_pam_screen(hipStream_t s, Pts X, int d, const int32_t* rows, const int64_t* crow, const int2* items,
                      int64_t nitems, const double* n2, const float* rho, double* St, double* Et,
                      const unsigned long long* cmax, unsigned long long* Sfix, unsigned long long* Efix) {
    if (nitems == 0) return 0;
    if (d > PAM_SCREEN_DMAX || nitems > 0x7fffffffll) {
        set_error("pam screen: unsupported shape");
        return -4;
    }
    return X.f64 ? pam_screen_tx(s, X.d(), d, rows, crow, items, nitems, n2, rho, St, Et, cmax, Sfix, Efix)
                 : pam_screen_tx(s, X.f(), d, rows, crow, items, nitems, n2, rho, St, Et, cmax, Sfix, Efix);
}

// One block per cluster: U = min_p (S~ + E) and the members that may still
// hold the minimum; a cluster that is not screened keeps every member.
__global__ __launch_bounds__(256) void pam_mark_kernel(const int64_t* __restrict__ crow,
                                                       const int32_t* __restrict__ screen,
                                                       const int* __restrict__ cbad, const double* __restrict__ St,
                                                       const double* __restrict__ Et,
                                                       const unsigned long long* __restrict__ cmax,
                                                       const unsigned long long* __restrict__ Sfix,
                                                       const unsigned long long* __restrict__ Efix,
                                                       uint8_t* __restrict__ flag,
                                                       int64_t* __restrict__ cnt,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ double red[4];
    __shared__ unsigned long long tot;
    const int c = blockIdx.x;
    const int64_t c0 = crow[c], c1 = crow[c + 1];
    if (!screen[c] || cbad[c]) {
        for (int64_t q = c0 + threadIdx.x; q < c1; q += 256) flag[q] = 1;
        if (threadIdx.x == 0) cnt[c] = c1 - c0;
        return;
    }
    const int n = (int)(c1 - c0);
    const double unit = 1.0 / pam_scale(cmax[c], n);
    double U = __builtin_inf();
    for (int64_t q = c0 + threadIdx.x; q < c1; q += 256) {
        double sv, ev;
        pam_total(q, St, Et, Sfix, Efix, unit, n, sv, ev);
        const double hi = sv + ev;
        if (hi < U) U = hi;                                  // a NaN never lowers it
    }
    for (int off = 32; off >= 1; off >>= 1) U = fmin(U, __shfl_xor(U, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = U;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    U = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    unsigned long long mine = 0;
    for (int64_t q = c0 + threadIdx.x; q < c1; q += 256) {
        double sv, ev;
        pam_total(q, St, Et, Sfix, Efix, unit, n, sv, ev);
        const bool keep = !(fabs(sv) < __builtin_inf() && fabs(ev) < __builtin_inf()) || sv - ev <= U;
        flag[q] = keep ? 1 : 0;
        mine += keep;
    }
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(&tot, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[c] = (int64_t)tot;
        atomicAdd(stats + STAT_PAM_SCREENED, 1ull);
        atomicAdd(stats + STAT_PAM_EXACT, tot);
    }
}

int launch_pam_mark(hipStream_t s, const int64_t* crow, int K, const int32_t* screen, const int* cbad,
                    const double* St, const double* Et, const unsigned long long* cmax,
                    const unsigned long long* Sfix, const unsigned long long* Efix, uint8_t* flag, int64_t* cnt,
                    unsigned long long* stats) {
    hipLaunchKernelGGL(pam_mark_kernel, dim3(K), dim3(256), 0, s, crow, screen, cbad, St, Et, cmax, Sfix, Efix, flag,
                       cnt, stats);
    return kstatus("pam_mark_kernel");
}

// One block per cluster: its flagged positions, in member order, from coff[c].
__global__ __launch_bounds__(256) void pam_compact_kernel(const int64_t* __restrict__ crow,
                                                          const uint8_t* __restrict__ flag,
                                                          const int64_t* __restrict__ coff,
                                                          int32_t* __restrict__ cand) {
    __shared__ int wcnt[4];
    const int c = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c0 = crow[c], c1 = crow[c + 1];
    int64_t base = coff[c];
    for (int64_t q0 = c0; q0 < c1; q0 += 256) {
        const int64_t q = q0 + threadIdx.x;
        const bool f = q < c1 && flag[q];
        const unsigned long long bal = __ballot(f);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 4; w++) {
            if (w < wave) before += wcnt[w];
            all += wcnt[w];
        }
        if (f) cand[base + before + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)q;
        base += all;
        __syncthreads();
    }
}

int launch_pam_compact(hipStream_t s, const int64_t* crow, int K, const uint8_t* flag, const int64_t* coff,
                       int32_t* cand) {
    hipLaunchKernelGGL(pam_compact_kernel, dim3(K), dim3(256), 0, s, crow, flag, coff, cand);
    return kstatus("pam_compact_kernel");
}

}  // namespace lshkm
