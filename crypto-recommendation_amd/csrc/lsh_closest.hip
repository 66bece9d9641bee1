// lsh_closest.hip — the MFMA screen of lshkm_lsh_p_closest:
// from a built cosine index straight to the few candidates per user that can
// be among its P closest, without ever writing a candidate list.
//
// A block owns LSHPC_COLS users as the f32 32x32x2 MFMA's B operand (32 per
// wave, one column per lane pair, in registers) and walks one segment of the
// pool rows, LSHPC_STAGE at a time through LDS (the A operand; pam.hip's
// layout and row stride). Row i is a candidate of user j iff some k-bit field
// of code_i ^ code_j is zero (they share a bucket in some table) and i is not
// in the excluded range. lshkm_cube_p_closest (§5e) runs the same kernel over a
// built hypercube: the codes are vertices and i is a candidate of j iff
// code_i ^ code_j is one of the probe masks (cubepc_member, lshpc_layout.h).
// For a candidate the screen has s~ = g~ / (|x^||u^|)
// and the interval [s~ - E, s~ + E] that holds the reference's similarity
// (the bound: §5c; E0 below is its part that no row or user changes).
//
// Every (user, segment) keeps a list of (row, lo, hi) of fixed capacity and a
// threshold T <= the (P+1)-th largest true similarity of the user: an entry is
// appended iff hi >= T. After a step, a list with more than cap - LSHPC_STAGE
// entries is pruned by its wave: T <- the (P+1)-th largest lo, entries with
// hi < T leave. A list still that full afterwards flags its user (overflow).
// What is appended depends only on T and the candidate, and T only on the set
// of entries at the step's end: no order of arrival changes the kept set.
#include "../../include/lshkm.h"
#include "common.h"
#include "kernels.h"
#include "lshpc_layout.h"

namespace lshkm {

typedef float floatx16 __attribute__((ext_vector_type(16)));

// The part of E every pair shares (§5c): (a) the MFMA chain, (c) the
// reference's own roundings (2^-40 covers (2 d + 16) 2^-53 for d <= 128 and the
// subnormal terms inside the magnitude range), (d) the f32 roundings of 1/|x^|,
// 1/|u^|, s~, E, lo and hi (< 2^-21; charged 2^-20).
template <int DP> constexpr float lshpc_e0() {
    return (float)(((DP + 8) * 0x1p-24 + 0x1p-20 + 0x1p-40) * (1.0 + 0x1p-20));
}

// Magnitude range the bound assumes: the reference's sum of squares within
// [2^-64, 2^64] (then no f32 operand, product or partial sum leaves the
// normal range by more than the 2^-40 term covers).
constexpr double LSHPC_XA_MIN = 0x1p-64, LSHPC_XA_MAX = 0x1p64;

// One wave per row: the f32 image x^ (zero-padded to dp), 1 / |x^| (negative:
// poison), the conversion term rel = 2.001 rho / |x^| (rho >= |x - x^|_2), the
// packed bucket code.
__global__ __launch_bounds__(256) void lshpc_prep_kernel(const double* __restrict__ X, int64_t n, int d, int dp,
                                                         const double* __restrict__ xa,
                                                         const int32_t* __restrict__ bucket, int L, int k,
                                                         float* __restrict__ xh, uint32_t* __restrict__ code,
                                                         float* __restrict__ inv, float* __restrict__ rel) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
        double s = 0.0, rr = 0.0;
        bool bad = false;
        for (int j = lane; j < dp; j += 64) {
            const double v = j < d ? X[(size_t)r * d + j] : 0.0;
            const float f = (float)v;
            const double fd = (double)f, dl = v - fd;
            bad |= !(fabs(v) < __builtin_inf());
            xh[(size_t)r * dp + j] = f;
            s = fma(fd, fd, s);
            rr = fma(dl, dl, rr);
        }
        for (int off = 32; off >= 1; off >>= 1) {
            s += __shfl_xor(s, off);
            rr += __shfl_xor(rr, off);
        }
        bad = __any(bad);
        const double a = xa[r];
        bad |= !(a >= LSHPC_XA_MIN && a <= LSHPC_XA_MAX) || !(s > 0.0);
        const double nrm = sqrt(s);
        const double relv = 2.001 * (sqrt(rr) * (1.0 + 0x1p-20)) / nrm;
        bad |= !(relv < 0x1p-12);
        if (lane == 0) {
            uint32_t c = 0;
            const uint32_t mask = k >= 32 ? 0xffffffffu : (1u << k) - 1u;
            for (int l = 0; l < L; l++) c |= ((uint32_t)bucket[(size_t)r * L + l] & mask) << (l * k);
            code[r] = c;
            inv[r] = bad ? -1.f : (float)(1.0 / nrm);
            rel[r] = bad ? 0.f : (float)relv * (1.f + 0x1p-20f);
        }
    }
}

// Order-preserving key of a non-NaN float.
__device__ inline uint32_t lshpc_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float lshpc_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Makes the wave's global stores visible to its other lanes.
__device__ inline void lshpc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The whole wave prunes one list of n entries (P + 1 <= n <= LSHPC_CAP_MAX):
// T <- max(T, the (P+1)-th largest lo), found by bisection on the keys' bits;
// entries with hi >= T stay, in list order. Returns the new count.
__device__ inline int lshpc_prune(float* klo, float* khi, int32_t* krow, int n, int P, int lane, float& T) {
    constexpr int PL = LSHPC_CAP_MAX / 64;
    float lo[PL], hi[PL];
    int32_t row[PL];
    uint32_t key[PL];
#pragma unroll
    for (int j = 0; j < PL; j++) {
        const int i = lane + 64 * j;
        const bool v = i < n;
        lo[j] = v ? klo[i] : 0.f;
        hi[j] = v ? khi[i] : 0.f;
        row[j] = v ? krow[i] : 0;
        key[j] = v ? lshpc_key(lo[j]) : 0u;      // below every real key
    }
    uint32_t cur = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t trial = cur | (1u << bit);
        int c = 0;
#pragma unroll
        for (int j = 0; j < PL; j++) c += __popcll(__ballot(key[j] >= trial));
        if (c >= P + 1) cur = trial;
    }
    T = fmaxf(T, lshpc_unkey(cur));
    int w = 0;
#pragma unroll
    for (int j = 0; j < PL; j++) {
        const bool keep = lane + 64 * j < n && hi[j] >= T;
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int p = w + __popcll(m & ((1ull << lane) - 1ull));
            klo[p] = lo[j];
            khi[p] = hi[j];
            krow[p] = row[j];
        }
        w += __popcll(m);
    }
    return w;
}

// CUBE = false: ca / cb = the lowest / highest bit of every table's field in the
// packed code (a field of code_i ^ code_j is zero iff the subtraction borrows
// out of it). CUBE = true: the codes are vertices and ca / cb = CubeProbe's
// shells / rev_last (lshpc_layout.h).
template <int DP, bool CUBE>
__global__ __launch_bounds__(256, 2) void lshpc_screen_kernel(LshpcSide rows, LshpcSide users, int32_t excl_lo,
                                                              int32_t excl_hi, int P, uint32_t ca, uint32_t cb,
                                                              LshpcKept kept) {
    constexpr int H = DP / 2;     // dims per lane half
    constexpr int DS = DP + 4;    // padded LDS row stride (floats): conflict-free ds_read_b128
    constexpr float E0 = lshpc_e0<DP>();
    __shared__ __attribute__((aligned(16))) float cs[LSHPC_STAGE * DS];
    __shared__ uint32_t rcode[LSHPC_STAGE];
    __shared__ float rinv[LSHPC_STAGE], rrel[LSHPC_STAGE];
    __shared__ int cnt[LSHPC_COLS], dead[LSHPC_COLS];
    __shared__ float Tl[LSHPC_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int ul = wave * 32 + col;                              // this lane's user of the block (both halves)
    const int64_t uq = (int64_t)blockIdx.x * LSHPC_COLS + ul;    // ... of the chunk (< kept.np)
    const bool own = uq < users.n;
    const int seg = blockIdx.y, cap = kept.cap;
    const size_t lbase = ((size_t)seg * kept.np + uq) * cap;

    float b[H];
#pragma unroll
    for (int s = 0; s < H; s++) b[s] = own ? users.xh[(size_t)uq * DP + h * H + s] : 0.f;
    const uint32_t ucode = own ? users.code[uq] : 0u;
    const float uinv = own ? users.inv[uq] : -1.f;
    const float urel = own ? users.rel[uq] : 0.f;
    if (threadIdx.x < LSHPC_COLS) {
        cnt[threadIdx.x] = 0;
        dead[threadIdx.x] = 0;
        Tl[threadIdx.x] = -__builtin_inff();
    }
    int seen = 0;
    bool pois = false;
    const int64_t r0 = (int64_t)seg * kept.seg_rows, r1 = min(rows.n, r0 + kept.seg_rows);
    // A step's rows are fetched into registers one step ahead (the loads fly
    // under the previous step's MFMAs) and stored to LDS at the step's top.
    constexpr int PRE = LSHPC_STAGE * DP / 4 / 256;      // float4 per thread and step
    float4 pre[PRE];
    uint32_t pcode = 0u;
    float pinv = 0.f, prel = 0.f;
    auto fetch = [&](int64_t m0) {
#pragma unroll
        for (int i = 0; i < PRE; i++) {
            const int e4 = threadIdx.x + 256 * i, r = e4 / (DP / 4), j = (e4 % (DP / 4)) * 4;
            pre[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m0 + r < r1) pre[i] = *reinterpret_cast<const float4*>(rows.xh + (size_t)(m0 + r) * DP + j);
        }
        if (threadIdx.x < LSHPC_STAGE) {
            const int64_t m = m0 + threadIdx.x;
            const bool in = m < r1 && !(m >= excl_lo && m < excl_hi);
            pcode = in ? rows.code[m] : 0u;
            pinv = in ? rows.inv[m] : 0.f;                     // 0: no one's candidate
            prel = in ? rows.rel[m] : 0.f;
        }
    };
    if (r0 < r1) fetch(r0);
    for (int64_t m0 = r0; m0 < r1; m0 += LSHPC_STAGE) {
#pragma unroll
        for (int i = 0; i < PRE; i++) {
            const int e4 = threadIdx.x + 256 * i, r = e4 / (DP / 4), j = (e4 % (DP / 4)) * 4;
            *reinterpret_cast<float4*>(cs + r * DS + j) = pre[i];
        }
        if (threadIdx.x < LSHPC_STAGE) {
            rcode[threadIdx.x] = pcode;
            rinv[threadIdx.x] = pinv;
            rrel[threadIdx.x] = prel;
        }
        __syncthreads();
        if (m0 + LSHPC_STAGE < r1) fetch(m0 + LSHPC_STAGE);
        const float T = Tl[ul];
        const bool alive = own && uinv > 0.f && !dead[ul];
#pragma unroll 1
        for (int t = 0; t < LSHPC_STAGE / 32; t++) {
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
                    const float inv = rinv[ml];
                    const uint32_t y = rcode[ml] ^ ucode;
                    const bool cand = CUBE ? cubepc_member(y, ca, cb) : ((y - ca) & ~y & cb) != 0u;
                    if (!own || inv == 0.f || !cand) continue;
                    seen++;
                    if (inv < 0.f) {
                        pois = true;
                    } else if (alive) {
                        const float s = acc[4 * g + q] * inv * uinv;
                        const float E = (E0 + rrel[ml]) + urel;
                        const float hi = s + E;
                        if (hi >= T) {
                            const int slot = atomicAdd(&cnt[ul], 1);
                            if (slot < cap) {                  // always (the invariant above); never out of bounds
                                kept.klo[lbase + slot] = s - E;
                                kept.khi[lbase + slot] = hi;
                                kept.krow[lbase + slot] = (int32_t)(m0 + ml);
                            }
                        }
                    }
                }
            }
        }
        // the step's end: this wave's lists that the next step could overflow
        lshpc_wave_sync();
        const bool last = m0 + LSHPC_STAGE >= r1;
        const int n_me = cnt[ul];
        const bool need = h == 0 && alive && (n_me > cap - LSHPC_STAGE || (last && n_me > P + 1));
        unsigned long long todo = __ballot(need);
        while (todo) {
            const int c = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int uc = wave * 32 + c;
            const size_t base = ((size_t)seg * kept.np + (size_t)blockIdx.x * LSHPC_COLS + uc) * cap;
            int n = min(cnt[uc], cap);
            float Tn = Tl[uc];
            const bool over_in = cnt[uc] > cap;
            n = lshpc_prune(kept.klo + base, kept.khi + base, kept.krow + base, n, P, lane, Tn);
            if (lane == 0) {
                cnt[uc] = n;
                Tl[uc] = Tn;
                if (over_in || n > cap - LSHPC_STAGE) dead[uc] = 1;      // overflow: the user goes to the lists
            }
        }
        __syncthreads();
    }
    if (r0 >= r1) __syncthreads();       // an empty segment: the initial state is what is written
    const int seen2 = seen + __shfl_xor(seen, 32);
    const int pois_other = __shfl_xor((int)pois, 32);        // every lane takes part: no short-circuit
    const bool pois2 = pois || pois_other != 0;
    if (own && h == 0) {
        const size_t st = (size_t)seg * kept.np + uq, plane = (size_t)kept.segs * kept.np;
        kept.state[st] = cnt[ul];
        kept.state[plane + st] = seen2;
        kept.state[2 * plane + st] = (int32_t)__float_as_uint(Tl[ul]);
        kept.state[3 * plane + st] = (dead[ul] || pois2 || !(uinv > 0.f)) ? 1 : 0;
    }
}

// One wave per user of the chunk: the segments' states joined. ncand = the
// candidates seen; flagged users (poison, overflow) keep nothing; the others
// keep the entries with hi >= T, T = the largest of the segments' thresholds
// raised once more over the joined list.
__global__ __launch_bounds__(256) void lshpc_count_kernel(LshpcKept kept, int64_t n, int P,
                                                          int64_t* __restrict__ nkept, int64_t* __restrict__ ncand,
                                                          unsigned long long* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const size_t plane = (size_t)kept.segs * kept.np;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (int64_t)gridDim.x * 4) {
        int flag = 0;
        int64_t seen = 0;
        float T = -__builtin_inff();
        for (int s = 0; s < kept.segs; s++) {
            const size_t st = (size_t)s * kept.np + q;
            flag |= kept.state[3 * plane + st];
            seen += kept.state[plane + st];
            T = fmaxf(T, __uint_as_float((uint32_t)kept.state[2 * plane + st]));
        }
        // entries with hi >= T; with bit >= 0, those of them whose lo's key is >= trial
        auto count = [&](float T, uint32_t trial, bool by_key) {
            int64_t total = 0;
            for (int s = 0; s < kept.segs; s++) {
                const size_t st = (size_t)s * kept.np + q;
                const int c = kept.state[st];
                const float *khi = kept.khi + st * kept.cap, *klo = kept.klo + st * kept.cap;
                for (int i0 = 0; i0 < c; i0 += 64) {
                    const int i = i0 + lane;
                    bool in = i < c && khi[i] >= T;
                    if (by_key) in = in && lshpc_key(klo[i]) >= trial;
                    total += __popcll(__ballot(in));
                }
            }
            return total;
        };
        int64_t total = 0;
        if (!flag) {
            total = count(T, 0u, false);
            if (kept.segs > 1 && total > P + 1) {
                // every segment kept its own P + 1 best: one more prune over the
                // joined list, T <- its (P+1)-th largest lo (a valid threshold too)
                uint32_t cur = 0;
                for (int bit = 31; bit >= 0; bit--) {
                    const uint32_t trial = cur | (1u << bit);
                    if (count(T, trial, true) >= P + 1) cur = trial;
                }
                T = fmaxf(T, lshpc_unkey(cur));
                total = count(T, 0u, false);
            }
        }
        if (lane == 0) {
            nkept[q] = total;
            if (ncand) ncand[q] = seen;
            atomicAdd(stats + STAT_LSHPC_SEEN, (unsigned long long)seen);
            atomicAdd(stats + STAT_LSHPC_KEPT, (unsigned long long)total);
        }
        lshpc_wave_sync();
        if (lane == 0) {                             // after every lane read the segments' flags
            kept.state[3 * plane + q] = flag;        // segment 0's slot: the user's flag
            kept.state[2 * plane + q] = (int32_t)__float_as_uint(T);
        }
    }
}

// One wave per unflagged user: its kept rows into cidx[cptr[q] ..), ascending
// (the segments are ascending row ranges; within one, by rank).
__global__ __launch_bounds__(256) void lshpc_fill_kernel(LshpcKept kept, int64_t n, const int64_t* __restrict__ cptr,
                                                         int32_t* __restrict__ cidx) {
    const int lane = threadIdx.x & 63;
    const size_t plane = (size_t)kept.segs * kept.np;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (int64_t)gridDim.x * 4) {
        if (kept.state[3 * plane + q]) continue;
        const float T = __uint_as_float((uint32_t)kept.state[2 * plane + q]);
        int64_t o = cptr[q];
        for (int s = 0; s < kept.segs; s++) {
            const size_t st = (size_t)s * kept.np + q;
            const int c = kept.state[st];
            const float* khi = kept.khi + st * kept.cap;
            const int32_t* krow = kept.krow + st * kept.cap;
            int kept_here = 0;
            for (int i0 = 0; i0 < c; i0 += 64) {
                const int i = i0 + lane;
                const bool mine = i < c && khi[i] >= T;
                if (mine) {
                    const int32_t r = krow[i];
                    int rank = 0;
                    for (int j = 0; j < c; j++) rank += (khi[j] >= T && krow[j] < r) ? 1 : 0;
                    cidx[o + rank] = r;
                }
                kept_here += __popcll(__ballot(mine));
            }
            o += kept_here;
        }
    }
}

// The users the screen hands back, appended to handed (any order; the host
// sorts): the flagged ones and the settle's replay list (a NaN or a tie).
__global__ __launch_bounds__(256) void lshpc_collect_kernel(LshpcKept kept, int64_t n, int64_t u0,
                                                            const int32_t* __restrict__ replay,
                                                            const unsigned int* __restrict__ replay_count,
                                                            int32_t* __restrict__ handed,
                                                            unsigned int* __restrict__ handed_count) {
    const size_t plane = (size_t)kept.segs * kept.np;
    const unsigned int nr = *replay_count;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
        if (kept.state[3 * plane + q]) handed[atomicAdd(handed_count, 1u)] = (int32_t)(u0 + q);
        if (q < nr) handed[atomicAdd(handed_count, 1u)] = (int32_t)(u0 + replay[q]);
    }
}

__global__ void lshpc_stats_kernel(unsigned long long* stats, unsigned long long settled, unsigned long long lists) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        stats[STAT_LSHPC_SETTLED] += settled;
        stats[STAT_LSHPC_LISTS] += lists;
    }
}

// The lists path's users, gathered: Ug[i] = U[list[i]].
__global__ __launch_bounds__(256) void lshpc_gather_kernel(const double* __restrict__ U, int d,
                                                           const int32_t* __restrict__ list, int64_t m,
                                                           double* __restrict__ Ug) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m * d; e += (int64_t)gridDim.x * 256)
        Ug[e] = U[(size_t)list[e / d] * d + e % d];
}

// lshkm_cube_p_closest's lists path, one thread per user of `list`: its vertex
// gathered and its combined bucket's length (the probed buckets' lengths).
__global__ __launch_bounds__(256) void cubepc_handed_kernel(const int32_t* __restrict__ vertex,
                                                            const int32_t* __restrict__ list, int64_t m,
                                                            const int32_t* __restrict__ masks, int S,
                                                            const int64_t* __restrict__ row_ptr,
                                                            int32_t* __restrict__ vg, int64_t* __restrict__ ncand) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
        const int32_t v = vertex[list[i]];
        int64_t n = 0;
        for (int j = 0; j < S; j++) {
            const int32_t b = v ^ masks[j];
            n += row_ptr[b + 1] - row_ptr[b];
        }
        vg[i] = v;
        ncand[i] = n;
    }
}

// ... and their results back to the users' slots.
__global__ __launch_bounds__(256) void lshpc_scatter_kernel(const int32_t* __restrict__ list, int64_t m, int P,
                                                            const int32_t* __restrict__ gidx,
                                                            const double* __restrict__ gsim,
                                                            const int32_t* __restrict__ gcnt,
                                                            const int64_t* __restrict__ eptr,
                                                            int32_t* __restrict__ out_idx, double* __restrict__ out_sim,
                                                            int32_t* __restrict__ out_cnt, int64_t* __restrict__ ncand) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m * P; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / P, j = e % P;
        const size_t u = (size_t)list[i];
        out_idx[u * P + j] = gidx[e];
        out_sim[u * P + j] = gsim[e];
        if (j == 0) {
            out_cnt[u] = gcnt[i];
            if (ncand) ncand[u] = eptr[i + 1] - eptr[i];
        }
    }
}

int launch_lshpc_prep(hipStream_t s, const double* X, int64_t n, int d, int dp, const double* xa, const int32_t* bucket,
                      int L, int k, const LshpcSide& out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lshpc_prep_kernel, dim3(gsz(n, 4, 8192)), dim3(256), 0, s, X, n, d, dp, xa, bucket, L, k,
                       const_cast<float*>(out.xh), const_cast<uint32_t*>(out.code), const_cast<float*>(out.inv),
                       const_cast<float*>(out.rel));
    return kstatus("lshpc_prep_kernel");
}

template <bool CUBE>
static int screen_launch(hipStream_t s, int dp, const LshpcSide& rows, const LshpcSide& users, int32_t excl_lo,
                         int32_t excl_hi, int P, uint32_t ca, uint32_t cb, const LshpcKept& kept) {
    if (kept.cap < P + 1 + LSHPC_STAGE || kept.cap > LSHPC_CAP_MAX || kept.np < users.n ||
        kept.np % LSHPC_COLS != 0 || (dp != 32 && dp != 128)) {
        set_error("lshpc screen: unsupported shape");
        return -4;
    }
    const dim3 grid((unsigned)(kept.np / LSHPC_COLS), (unsigned)kept.segs), block(256);
    if (dp == 32)
        hipLaunchKernelGGL((lshpc_screen_kernel<32, CUBE>), grid, block, 0, s, rows, users, excl_lo, excl_hi, P, ca, cb, kept);
    else
        hipLaunchKernelGGL((lshpc_screen_kernel<128, CUBE>), grid, block, 0, s, rows, users, excl_lo, excl_hi, P, ca, cb, kept);
    return kstatus("lshpc_screen_kernel");
}

int launch_lshpc_screen(hipStream_t s, int dp, const LshpcSide& rows, const LshpcSide& users, int32_t excl_lo,
                        int32_t excl_hi, int P, int L, int k, const LshpcKept& kept) {
    if (users.n <= 0) return 0;
    if (L < 1 || k < 1 || (int64_t)L * k > 32) {
        set_error("lshpc screen: unsupported shape");
        return -4;
    }
    uint32_t lowb = 0;
    for (int l = 0; l < L; l++) lowb |= 1u << (l * k);
    const uint32_t highb = lowb << (k - 1);
    return screen_launch<false>(s, dp, rows, users, excl_lo, excl_hi, P, lowb, highb, kept);
}

int launch_cubepc_screen(hipStream_t s, int dp, const LshpcSide& rows, const LshpcSide& users, int P,
                         const CubeProbe& probe, const LshpcKept& kept) {
    if (users.n <= 0) return 0;
    return screen_launch<true>(s, dp, rows, users, 0, 0, P, probe.shells, probe.rev_last, kept);
}

int launch_lshpc_join(hipStream_t s, const LshpcKept& kept, int64_t n, int P, int64_t* nkept, int64_t* ncand,
                      int64_t* cptr, int32_t* cidx, unsigned long long* stats) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lshpc_count_kernel, dim3(gsz(n, 4, 8192)), dim3(256), 0, s, kept, n, P, nkept, ncand, stats);
    int rc;
    if ((rc = launch_scan_i64(s, nkept, n, cptr))) return rc;
    hipLaunchKernelGGL(lshpc_fill_kernel, dim3(gsz(n, 4, 8192)), dim3(256), 0, s, kept, n, cptr, cidx);
    return kstatus("lshpc_fill_kernel");
}

int launch_lshpc_collect(hipStream_t s, const LshpcKept& kept, int64_t n, int64_t u0, const int32_t* replay,
                         const unsigned int* replay_count, int32_t* handed, unsigned int* handed_count) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lshpc_collect_kernel, dim3(gsz(n, 256, 1024)), dim3(256), 0, s, kept, n, u0, replay, replay_count,
                       handed, handed_count);
    return kstatus("lshpc_collect_kernel");
}

int launch_lshpc_stats(hipStream_t s, unsigned long long* stats, int64_t settled, int64_t lists) {
    hipLaunchKernelGGL(lshpc_stats_kernel, dim3(1), dim3(64), 0, s, stats, (unsigned long long)settled,
                       (unsigned long long)lists);
    return kstatus("lshpc_stats_kernel");
}

int launch_lshpc_gather(hipStream_t s, const double* U, int d, const int32_t* list, int64_t m, double* Ug) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(lshpc_gather_kernel, dim3(gsz(m * d, 256, 8192)), dim3(256), 0, s, U, d, list, m, Ug);
    return kstatus("lshpc_gather_kernel");
}

int launch_cubepc_handed(hipStream_t s, const int32_t* vertex, const int32_t* list, int64_t m, const int32_t* masks,
                         int S, const int64_t* row_ptr, int32_t* vg, int64_t* ncand) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(cubepc_handed_kernel, dim3(gsz(m, 256, 8192)), dim3(256), 0, s, vertex, list, m, masks, S, row_ptr,
                       vg, ncand);
    return kstatus("cubepc_handed_kernel");
}

int launch_lshpc_scatter(hipStream_t s, const int32_t* list, int64_t m, int P, const int32_t* gidx, const double* gsim,
                         const int32_t* gcnt, const int64_t* eptr, int32_t* out_idx, double* out_sim, int32_t* out_cnt,
                         int64_t* ncand) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(lshpc_scatter_kernel, dim3(gsz(m * P, 256, 8192)), dim3(256), 0, s, list, m, P, gidx, gsim, gcnt,
                       eptr, out_idx, out_sim, out_cnt, ncand);
    return kstatus("lshpc_scatter_kernel");
}

}  // namespace lshkm
