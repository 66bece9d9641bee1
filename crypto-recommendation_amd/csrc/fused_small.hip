// fused_small.hip — the small kernels around the fused pass (fused.hip): the
// centroid preparation, the hash fix-up, the winners' distance fix-up and the
// fp64 rows' sums of squares, each with its launcher.
#include "fused_impl.h"

namespace lshkm {

// Rows listed by the fused pass with an uncertified floor (euclidean) or sign
// (cosine): fix-up pass. Eight lanes per listed row. In load u of a row the
// group reads 128 contiguous bytes (lane q the 16 at dims 32u + 4q), so one
// load instruction covers one whole line of each of the wave's 8 rows and a
// row's four lines are visited once each; lane q ends up with dims
// {32u + 4q + i}, u < 4, i < 4. With k = 4 (the only k the persistent form
// hashes with; L <= 8) lane q also holds one whole table, tuples [4q, 4q + 4).
// Sixteen row registers per lane instead of 32 (two rows are held: the next
// row of the group is loaded while the current one is computed) keep the
// kernel under 128 VGPRs, 4 waves per SIMD, and the kernel lives on latency.
// The projections and per-function constants sit in LDS, so the only global
// latency per row is the prefetched one.
//
// Exactness. The fp64 products are summed per lane and then across the 8
// lanes, so acc may differ in its last bits from any other order; hash.hip's
// bound covers every summation order of the 128 products (depth 9 < 130).
// A floor or sign the bound certifies is therefore the reference's; an
// uncertified one goes to the soft-x87 chain, which walks the dims in the
// reference's order (only its index into the LDS image follows the lanes'
// layout). Tuples, phi and buckets are bit-identical whatever the layout;
// only the diagnostic STAT_HASH_EXACT may move.
constexpr int HF_WAVES = 4;
constexpr int HF_SPLIT = 4;                           // blocks per list segment
constexpr int HF_G = 8;                               // lanes per listed row
constexpr int HF_SLOTS = 64 * HF_WAVES / HF_G;        // rows per block pass
constexpr int HF_XL = FU_D / HF_G;                    // dims per lane
// LDS image of the projections (fp64): lane q's j-th value (dim 32(j / 4) + 4q +
// j % 4) at q * HF_QS + j * HF_PS; the lanes' parts skewed by 4 doubles (q *
// HF_QS = 20q double-banks mod 32: eight different ones) so that the 8 lanes
// of a row, reading their j-th dim of the same function, hit different banks
// (LK <= 32)
constexpr int HF_PS = 33;
constexpr int HF_QS = HF_XL * HF_PS + 4;
constexpr size_t HF_LDS = (size_t)HF_G * HF_QS * 8 + 32 * (8 + 8 + 4);
__device__ inline int hf_pidx(int r) { return ((r >> 2) & 7) * HF_QS + (((r >> 5) << 2) | (r & 3)) * HF_PS; }

// lane ^ 1 / lane ^ 2 within each quad by DPP quad_perm, lane i <-> 7 - i
// within each 8 lanes by row_half_mirror (VALU moves)
template <int CTRL>
__device__ inline uint32_t dpp_move(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ inline double dpp_move(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint64_t lo = dpp_move<CTRL>((uint32_t)b), hi = dpp_move<CTRL>((uint32_t)(b >> 32));
    return __longlong_as_double((long long)((hi << 32) | lo));
}
template <int CTRL>
__device__ inline float dpp_move(float v) { return __uint_as_float(dpp_move<CTRL>(__float_as_uint(v))); }
constexpr int QP_X1 = 0xB1, QP_X2 = 0x4E, HALF_MIRROR = 0x141;   // quad_perm [1,0,3,2], [2,3,0,1]; row_half_mirror
// sum over the 8 lanes of a row group (all active together); every lane gets
// the same value (((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)) in any
// lane's operand order: the mirror pairs a lane with one of the other quad)
template <typename T>
__device__ inline T group_sum(T v) {
    v += dpp_move<QP_X1>(v);
    v += dpp_move<QP_X2>(v);
    v += dpp_move<HALF_MIRROR>(v);
    return v;
}

// the rare sequential fallbacks, out of line (their registers would lower the
// occupancy of the whole kernel)
__device__ __noinline__ int32_t fixup_floor_x87(const float* xrow, const double* pts, int f, double tt, float w) {
    return hash_x87_floor([&](int j) { return pts[hf_pidx(j) + f]; }, xrow, FU_D, tt, w);
}
__device__ __noinline__ int fixup_sign_x87(const float* xrow, const double* pts, int f) {
    return hash_x87_sign([&](int j) { return pts[hf_pidx(j) + f]; }, xrow, FU_D);
}

// One listed row as the group's lane q holds it.
struct FixRow {
    int64_t row;
    uint32_t mask;
    float x[HF_XL];    // x[4u + i] = dim 32u + 4q + i
    int32_t v[4];      // euclidean: table q's tuples [4q, 4q + 4); cosine: v[0] = g of table q
};

// One table's 4 tuples (k = 4) as one 16-B access of 4-B alignment: a caller's
// tuple buffer need not be 16-B aligned.
struct alignas(4) Tup4 { int32_t v[4]; };

template <bool COS>
__device__ inline void fix_load(const FusedArgs& a, unsigned long long ent, int q, FixRow& r) {
    r.row = (int64_t)(ent >> 32);
    r.mask = (uint32_t)ent;
    const float* xq = a.X + r.row * FU_D + 4 * q;
#pragma unroll
    for (int u = 0; u < HF_XL / 4; u++) {
        const float4 v = *reinterpret_cast<const float4*>(xq + 32 * u);
        r.x[4 * u] = v.x; r.x[4 * u + 1] = v.y; r.x[4 * u + 2] = v.z; r.x[4 * u + 3] = v.w;
    }
    // unconditional loads (clamped indices; the extra values are never used):
    // a load under a branch makes the compiler wait for it at the merge
    const int l = min(q, a.L - 1);
    if (COS) {
        r.v[0] = ((a.bucket ? a.bucket : a.phi) + r.row * a.L)[l];
    } else {
        const Tup4 v = reinterpret_cast<const Tup4*>(a.tuples + r.row * a.LK)[l];
#pragma unroll
        for (int j = 0; j < 4; j++) r.v[j] = v.v[j];
    }
}

template <bool COS>
__device__ inline void fix_row(const FusedArgs& a, const double* pts, const double* cpn, const double* ctt, int q,
                               FixRow& r) {
    // nx >= |x| only bounds, so it is summed in f32 and rounded up (the fp64 form
    // cost a widening and an fp64 FMA per dim and an fp64 sqrt per row). The
    // terms are non-negative and the sum is 9 roundings deep: s >= |x|^2 (1 -
    // 2^-20) less what underflows, < 40 * 2^-126 even with denormals flushed; so
    // |x|^2 <= s (1 + 2^-15) + 2^-118, whose v_sqrt_f32 (1 ulp) is covered by
    // 1 + 2^-20. An overflowing or non-finite row gives inf / NaN, no certificate.
    float xs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < HF_XL; j++) xs[j & 3] = fmaf(r.x[j], r.x[j], xs[j & 3]);
    const float s = group_sum((xs[0] + xs[1]) + (xs[2] + xs[3]));
    const double nx = (double)__builtin_amdgcn_sqrtf(fmaf(s, 1.f + 0x1p-15f, 0x1p-118f)) * (1.0 + 0x1p-20);
    const float* xrow = a.X + r.row * FU_D;
    const int k = a.k;
    const double iwd = 1.0 / (double)a.w;
    for (uint32_t m = r.mask; m; m &= m - 1) {
        const int f = __builtin_ctz(m);
        const double* pq = pts + q * HF_QS + f;
        // the dot product: four independent accumulators per lane (one fp64 FMA
        // chain left the waves issue-stalled on its dependencies); its bound
        // covers any summation order
        double aq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < HF_XL; j++) aq[j & 3] = fma(pq[j * HF_PS], (double)r.x[j], aq[j & 3]);
        const double acc = group_sum((aq[0] + aq[1]) + (aq[2] + aq[3]));
        const double P = cpn[f] * nx * (1.0 + 0x1p-40);
        if (COS) {
            int bit;
            if (!hash_decide_sign(acc, P, FU_D, bit)) {   // the same decision in all 8 lanes
                bit = fixup_sign_x87(xrow, pts, f);
                if (q == 0) atomicAdd(a.stats + STAT_HASH_EXACT, 1ull);
            }
            // g = bits MSB first (CosineGGen): function l*k + i is bit k-1-i of table l
            const int l = f / k, b = 1 << (k - 1 - (f - l * k));
            if (l == q) r.v[0] = bit ? (r.v[0] | b) : (r.v[0] & ~b);
        } else {
            // y by the reciprocal (iw = RN(1/w)): three roundings of 2^-53 each
            // relative, inside the |y| 2^-50 term
            const double tt = ctt[f], iw = iwd;
            const double y = (acc + tt) * iw;
            const double B = ((double)(FU_D + 2) * 0x1p-52 * (P + fabs(tt))) * (iw * (1.0 + 0x1p-50)) +
                             fabs(y) * 0x1p-50;
            const double lo = floor(y - B), hi = floor(y + B);
            int32_t hv = (int32_t)lo;
            // outside the int range the reference's FISTP stores INT_MIN: the x87 form
            if (!(lo == hi && fabs(lo) < 0x1p31)) {  // the same decision in all 8 lanes
                hv = fixup_floor_x87(xrow, pts, f, tt, a.w);
                if (q == 0) atomicAdd(a.stats + STAT_HASH_EXACT, 1ull);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) r.v[i] = f == 4 * q + i ? hv : r.v[i];
        }
    }
}

// Wait here for a row's loads (and the list entry loaded after them). The
// vector-memory counter retires in order and the number of a row's stores
// varies, so a wait for the next row's loads placed after the current row's
// stores also waits for those stores' acknowledgements. The loop waits between
// the computation and the stores instead: the loads have had the whole
// computation to land, and the stores stay in flight through the next row's
// computation.
__device__ inline void fix_settle(FixRow& r, unsigned long long& ent) {
    asm volatile("" : "+v"(r.row), "+v"(r.mask), "+v"(ent));
#pragma unroll
    for (int j = 0; j < HF_XL; j++) asm volatile("" : "+v"(r.x[j]));
#pragma unroll
    for (int j = 0; j < 4; j++) asm volatile("" : "+v"(r.v[j]));
}

// The row's stores, apart from its computation: the kernel's loop waits for the
// next row's loads between the two (fix_settle). k = 4 (fused_route sends
// every other k to the chunked form): lane q's tuples [4q, 4q + 4) are the
// whole table q, so each lane stores its own table where touched, tuples (the
// unflagged ones as loaded) and phi / bucket, with no sum across lanes and no
// loop over the tables for the whole wave.
template <bool COS>
__device__ inline void fix_store(const FusedArgs& a, const int32_t* crv, int q, const FixRow& r) {
    const int k = a.k;
    const uint32_t kmask = k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
    const bool touched = q < a.L && (r.mask & (kmask << (q * k)));
    if (COS) {
        if (touched) {
            if (a.phi) a.phi[r.row * a.L + q] = r.v[0];
            if (a.bucket) a.bucket[r.row * a.L + q] = r.v[0];
        }
        return;
    }
    // the uint32 sum of the phi terms wraps the same in any order; computed in
    // every lane (tables >= L hold clamped loads), stored where touched
    uint32_t hn = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) hn += phi_term(r.v[j], crv[4 * q + j]);
    if (touched) {
        Tup4 v;
#pragma unroll
        for (int j = 0; j < 4; j++) v.v[j] = r.v[j];
        *reinterpret_cast<Tup4*>(a.tuples + r.row * a.LK + 4 * q) = v;
        const uint32_t ph = phi_final(hn);
        if (a.phi) a.phi[r.row * a.L + q] = (int32_t)ph;
        if (a.bucket) a.bucket[r.row * a.L + q] = bucket_fast(ph, a.bdiv);
    }
}

template <bool COS>
__global__ __launch_bounds__(64 * HF_WAVES) void hash_fixup_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* pts = reinterpret_cast<double*>(smem);   // skewed [128][32]
    double* cpn = pts + HF_G * HF_QS;                // [32] |p_f| (rounded up)
    double* ctt = cpn + 32;                          // [32] t_f
    int32_t* crv = reinterpret_cast<int32_t*>(ctt + 32);   // [32] r_f
    const int nseg = gridDim.x / HF_SPLIT;       // segments across XCDs (cos_fix_seg_kernel)
    const int seg = blockIdx.x % nseg, part = blockIdx.x / nseg;
    const int n = a.seg_counts[SEG_SLOTS * seg + SEG_FIX];
    if (n == 0) return;                                                 // block-uniform
    const unsigned long long* list = a.hfix + (int64_t)seg * a.seg_rows;
    const int LK = a.LK, LKpad = a.LKpad;
    // constant trip count and clamped, unconditional loads: all 16 in flight
    // together (a loop over e < FU_D * 32 with the load under f < LK stayed
    // rolled, one L2 round trip per step)
    {
        const int f = threadIdx.x & 31, fc = min(f, LKpad - 1);
        double pv[FU_D * 32 / (64 * HF_WAVES)];
#pragma unroll
        for (int i = 0; i < FU_D * 32 / (64 * HF_WAVES); i++)
            pv[i] = a.PT[((threadIdx.x >> 5) + i * (2 * HF_WAVES)) * LKpad + fc];
#pragma unroll
        for (int i = 0; i < FU_D * 32 / (64 * HF_WAVES); i++)
            pts[hf_pidx((threadIdx.x >> 5) + i * (2 * HF_WAVES)) + f] = f < LK ? pv[i] : 0.0;
    }
    if (threadIdx.x < 32) {
        const int f = threadIdx.x;
        cpn[f] = f < LK ? a.pnorm[f] : 0.0;
        ctt[f] = !COS && f < LK ? (double)a.tv[f] : 0.0;
        crv[f] = !COS && f < LK ? a.rv[f] : 0;
    }
    __syncthreads();
    const int q = threadIdx.x & (HF_G - 1), slot = threadIdx.x / HF_G;
    constexpr int STRIDE = HF_SPLIT * HF_SLOTS;
    int e = part * HF_SLOTS + slot;
    if (e >= n) return;                                                 // whole groups
    // software pipeline: the next row (and the list entry after it) load while
    // the current one is computed; past the end the last entry is re-loaded
    FixRow cur, nxt;
    fix_load<COS>(a, list[e], q, cur);
    unsigned long long ent2 = list[min(e + STRIDE, n - 1)];
    fix_settle(cur, ent2);
    for (; e < n; e += STRIDE) {
        fix_load<COS>(a, ent2, q, nxt);
        ent2 = list[min(e + 2 * STRIDE, n - 1)];
        fix_row<COS>(a, pts, cpn, ctt, q, cur);
        fix_settle(nxt, ent2);
        fix_store<COS>(a, crv, q, cur);
        cur = nxt;
    }
}

void launch_hash_fixup(hipStream_t s, const RecList& l, bool cosine, FusedArgs a) {
    a.hfix = l.p; a.seg_counts = l.counts; a.seg_rows = l.seg_rows;
    const unsigned nseg = (unsigned)l.nseg;
    const dim3 grid(nseg * HF_SPLIT), block(64 * HF_WAVES);
    if (cosine) hipLaunchKernelGGL(hash_fixup_kernel<true>, grid, block, HF_LDS, s, a);
    else hipLaunchKernelGGL(hash_fixup_kernel<false>, grid, block, HF_LDS, s, a);
}

// ------------------------------------------------------------------ preparation
// Centroids -> f16 hi/lo rows, -||c||^2/2, and the per-call bound maxima.
constexpr int FP_PREP_WAVES = 8;     // centroids per prep block (Kpad % 64 == 0)
// d < 128: the rows are zero-padded to 128 dims (C64p: the padded fp64 copy the
// winner chains read; a zero dim adds (0 - 0)^2 = +0 to a non-negative chain).
__global__ void fused_centroid_prep(const double* __restrict__ C, int K, int Kpad, _Float16* __restrict__ Ch,
                                    _Float16* __restrict__ Cl, float* __restrict__ cnh, unsigned int* __restrict__ cb,
                                    int metric, double* __restrict__ nbv, float* __restrict__ C32,
                                    float* __restrict__ rn32, int d, double* __restrict__ C64p) {
    const int c = blockIdx.x * FP_PREP_WAVES + (threadIdx.x >> 6);   // one wave per centroid row
    const int lane = threadIdx.x & 63;
    double s2 = 0.0, s1 = 0.0;
    bool bad = false;
    double scale = 1.0;                  // cosine: the row is normalised (score x.c/|c|)
    if (metric == 1) {
        double q = 0.0;
        for (int j = lane; j < FU_D; j += 64) {
            const double v = c < K && j < d ? C[(size_t)c * d + j] : 0.0;
            q = fma(v, v, q);
        }
        for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off);
        // zero / extreme-norm centroids (the reference's NaN for a zero vector,
        // assignment.hpp:66) leave the call uncertified: every row goes exact
        if (c < K && !(q >= 1e-200 && q <= 1e200)) bad = true;
        scale = (q >= 1e-200 && q <= 1e200) ? 1.0 / sqrt(q) : 0.0;
        if (lane == 0 && c < K) {
            double b = 0.0;
            for (int j = 0; j < d; j++) {
                const double cj = C[(size_t)c * d + j];
                b = __dadd_rn(b, gp_sq(cj));
            }
            nbv[c] = b;
        }
    }
    bool not32 = false;                  // some value of the row is not an f32 (cbound[7] bit 0)
    bool tiny = false;                   // some 0 < |c_j| < 2^-460 (cbound[7] bit 1: PwAcc)
    double rr = 0.0, hh = 0.0;           // |c - ch|^2, |ch|^2 (the hi-only scores' bound)
    double r32 = 0.0;                    // |c - f32(c)|^2 (fast distances)
    for (int j = lane; j < FU_D; j += 64) {
        const double raw = c < K && j < d ? C[(size_t)c * d + j] : 0.0;
        const double v = raw * scale;
        if (C64p) C64p[(size_t)c * FU_D + j] = raw;
        const float f = (float)v;
        not32 |= c < K && (double)f != v;
        tiny |= c < K && fabs(raw) < 0x1p-460 && raw != 0.0;
        if (C32) {
            C32[(size_t)c * FU_D + j] = f;
            const double e = v - (double)f;       // exact (or inf / nan: never certified)
            r32 = fma(e, e, r32);
        }
        const _Float16 hv = (_Float16)f;
        Ch[(size_t)c * FU_D + j] = hv;
        Cl[(size_t)c * FU_D + j] = (_Float16)(f - (float)hv);
        s2 = fma(v, v, s2);
        s1 += fabs(v);
        const double r = v - (double)hv;     // exact in fp64 for |v| <= 2^15
        rr = fma(r, r, rr);
        hh = fma((double)hv, (double)hv, hh);
        bad |= !(fabs(v) <= (double)FU_RANGE);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        s2 += __shfl_xor(s2, off);
        s1 += __shfl_xor(s1, off);
        rr += __shfl_xor(rr, off);
        hh += __shfl_xor(hh, off);
        r32 += __shfl_xor(r32, off);
    }
    // sum of 128 non-negative fp64 values: <= 2^-46 relative rounding; rounded up
    if (rn32 && lane == 0) rn32[c] = r32 == 0.0 ? 0.f : (float)(sqrt(r32) * (1.0 + 0x1p-40)) * (1.f + 0x1p-22f);
    const unsigned long long anybad = __ballot(bad);
    const unsigned long long any_not32 = __ballot(not32);
    const unsigned long long any_tiny = __ballot(tiny);
    // per wave (centroid) the bound maxima, then one atomic per word per block:
    // single-word atomics from every centroid serialise (~12 ns each)
    __shared__ unsigned int wmax[FP_PREP_WAVES][8];
    if (lane == 0) {
        unsigned int m[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        m[7] = (any_not32 ? 1u : 0u) | (any_tiny ? 2u : 0u);
        if (c >= K) {
            // padding rows: a finite score far below any real one (|x.c| < 2^38 under
            // the range guard), so the packed-index trick never meets an inf/nan
            cnh[c] = -0x1p100f;
        } else {
            cnh[c] = metric == 1 ? 0.f : (float)(-0.5 * s2);
            const double up = 1.0 + 0x1p-18;
            const double nc = sqrt(s2) * (1.0 + 0x1p-30);
            // |t~ - t| <= (A1 + 2^-22)|x||c| + A2(|x|_1 + |c|_1) + 2^-23 |c|^2 + 2^-41 (|x|^2 + |c|^2)
            // (cosine: no |c|^2 term in t, c = the normalised row)
            m[0] = __float_as_uint((float)((FU_A1 + 0x1p-22) * nc * up));     // positive floats order like their bits
            m[1] = __float_as_uint((float)((FU_A2 * s1 * (1.0 + 0x1p-20) + (metric == 1 ? 0.0 : 0x1p-23 * s2) +
                                            0x1p-41 * s2) * up));
            m[2] = anybad ? 1u : 0u;
            m[3] = __float_as_uint((float)(nc * up));                        // max |c|, rounded up
            // hi-only scores (fused_hi_kernel): max |c - ch|, max |ch|, max |cn|, rounded up
            m[4] = __float_as_uint((float)(sqrt(rr) * (1.0 + 0x1p-30) * up));
            m[5] = __float_as_uint((float)(sqrt(hh) * (1.0 + 0x1p-30) * up));
            m[6] = __float_as_uint((float)(metric == 1 ? 0.0 : 0.5 * s2 * up));
        }
#pragma unroll
        for (int i = 0; i < 8; i++) wmax[threadIdx.x >> 6][i] = m[i];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int i = threadIdx.x;
        unsigned int v = 0u;
        for (int w = 0; w < FP_PREP_WAVES; w++) v = i == 2 || i == 7 ? (v | wmax[w][i]) : max(v, wmax[w][i]);
        if (v) {
            if (i == 2 || i == 7) atomicOr(cb + i, v);
            else atomicMax(cb + i, v);
        }
    }
}

int launch_fused_prep(hipStream_t s, const double* C, int K, int d, int metric, const FusedWorkspace& w) {
    const int Kpad = (K + 63) / 64 * 64;
    static_assert(64 % FP_PREP_WAVES == 0, "Kpad is a multiple of 64");
    // (w.cbound's FUSED_CBOUND_BYTES are zero here: fused_assign's clear, or the last call's epilogue)
    hipLaunchKernelGGL(fused_centroid_prep, dim3((unsigned)(Kpad / FP_PREP_WAVES)), dim3(64 * FP_PREP_WAVES), 0, s, C, K, Kpad, w.Ch, w.Cl, w.cnh,
                       reinterpret_cast<unsigned int*>(w.cbound), metric, w.nbv, w.C32, w.rn32, d, w.C64p);
    return kstatus("fused_centroid_prep");
}

// Winners listed by the fused kernels for their distance alone: lane per row.
// Cosine (MET = 1): the certificate declined, the x87 chain decides
// (exact_cosine_x87_wave). Euclidean (MET = 0, exact distances): a square of
// the chain was inexact, so glibc's pow(x, 2) may differ from x*x -- the chain
// again with glibc's pow (exact_euclid_wave). CF_SPLIT blocks per list segment; both
// lists of a call (the hi-only pass's and the refinement's) in ONE launch, so
// the short list's lone chains (~40 us of latency) overlap the long one.
constexpr int CF_SPLIT = 8;
struct CosLists {
    const unsigned long long* list[2];
    const int32_t* counts[2];
};
template <typename TX, int MET>
__global__ __launch_bounds__(256) void cos_fix_seg_kernel(const TX* __restrict__ X, int d, const double* __restrict__ C,
                                                          CosLists cl, int nseg, int64_t seg_rows,
                                                          const int32_t* __restrict__ assign, double* __restrict__ dist,
                                                          const double* __restrict__ xn2, const double* __restrict__ nbv) {
    // consecutive blocks take different segments: blocks are dealt round-robin to
    // the 8 XCDs, and a short list fills only its segment's first part (with
    // seg = blockIdx / CF_SPLIT every busy block sat on one XCD: 4x slower)
    const int per_list = nseg * CF_SPLIT;
    const int li = blockIdx.x / per_list, b = blockIdx.x % per_list;
    const int seg = b % nseg, part = b / nseg;
    const int n = cl.counts[li][SEG_SLOTS * seg + SEG_FIX];
    const unsigned long long* l = cl.list[li] + (int64_t)seg * seg_rows;
    const bool vec = sizeof(TX) == 4 && d % 8 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)C & 15) == 0;
    __shared__ double sqs[4][64 * 16];                   // gp_sq_wave: 64 * NV per wave
    double* sq = sqs[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    // wave-uniform trip count (the chains run the whole wave in step); a lane
    // past the list end repeats the wave's first row and writes nothing
    for (int i0 = part * 256 + (threadIdx.x & ~63); i0 < n; i0 += CF_SPLIT * 256) {
        const int i = i0 + lane;
        const bool live = i < n;
        const int64_t row = (int64_t)l[live ? i : i0];
        const TX* xr = X + row * d;
        const double* cr = C + (size_t)assign[row] * d;
        double v;
        if constexpr (MET == 1) {
            // the sums of squares precomputed (the prep's nbv; fp64 rows: row_sumsq)
            // when the launch has them: no squares left in the chain
            if (nbv && (sizeof(TX) == 4 || xn2)) {
                const double xa = sizeof(TX) == 4 ? -1.0 : xn2[row], cb = nbv[assign[row]];
                if (vec) v = exact_cosine_x87_pf<sizeof(TX) == 4>(xr, cr, d, xa, cb);
                else v = exact_cosine_x87_pf<false>(xr, cr, d, xa, cb);
            } else if (vec) {
                v = exact_cosine_x87_wave<sizeof(TX) == 4>(xr, cr, d, sq);
            } else {
                v = exact_cosine_x87_wave<false>(xr, cr, d, sq);
            }
        } else {
            if (vec) v = exact_euclid_wave<sizeof(TX) == 4>(xr, cr, d, sq);
            else v = exact_euclid_wave<false>(xr, cr, d, sq);
        }
        if (live) dist[row] = v;
    }
}

// out[i] = the reference's sum_j pow(x_ij, 2), j ascending (the |x|^2 of
// cosineDistance, cust_vector.hpp:148-151) for fp64 rows, lane per row. A wave
// takes 64 rows; VEC (d even, rows 16-B aligned): each 8-dim step of the 64
// rows is loaded as 16-B pieces, four lanes per row's 64 contiguous bytes, and
// transposed through LDS (a lane-per-row load touches 64 lines per instruction).
constexpr int RSQ_S = 10;                                // LDS row stride (doubles)
template <bool VEC>
__global__ __launch_bounds__(256) void row_sumsq_kernel(const double* __restrict__ X, int64_t N, int d,
                                                         double* __restrict__ out) {
    __shared__ double sqs[4][64 * 8];                    // gp_sq_wave: 64 * NV per wave
    __shared__ __attribute__((aligned(16))) double tr[4][64 * RSQ_S];
    double* sq = sqs[threadIdx.x >> 6];
    double* t = tr[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    // wave-uniform trip count: lanes past N repeat row N - 1 and write nothing
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); i0 < N; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + lane;
        double a = 0.0;
        if constexpr (VEC) {
            double2 pc[4], pn[4];
            auto load = [&](int j0, double2 (&dst)[4]) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int q = 64 * k + lane, r = q >> 2, part = q & 3;
                    const int64_t rr = i0 + r < N ? i0 + r : N - 1;
                    const int j = j0 + 2 * part;
                    dst[k] = j < d ? *reinterpret_cast<const double2*>(X + rr * d + j) : make_double2(0.0, 0.0);
                }
            };
            load(0, pn);
            for (int j0 = 0; j0 < d; j0 += 8) {
#pragma unroll
                for (int k = 0; k < 4; k++) pc[k] = pn[k];
                if (j0 + 8 < d) load(j0 + 8, pn);               // the next step in flight
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int q = 64 * k + lane;
                    *reinterpret_cast<double2*>(t + (q >> 2) * RSQ_S + 2 * (q & 3)) = pc[k];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                double v[8], p[8];
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const double2 w = *reinterpret_cast<const double2*>(t + lane * RSQ_S + 2 * h);
                    v[2 * h] = w.x;
                    v[2 * h + 1] = w.y;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                gp_sq_wave<8>(v, p, sq);
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (j0 + u < d) a = __dadd_rn(a, p[u]);
            }
        } else {
            const double* x = X + (i < N ? i : N - 1) * d;
            for (int j0 = 0; j0 < d; j0 += 8) {
                double v[8], p[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = j0 + u < d ? x[j0 + u] : 0.0;
                gp_sq_wave<8>(v, p, sq);
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (j0 + u < d) a = __dadd_rn(a, p[u]);
            }
        }
        if (i < N) out[i] = a;
    }
}

int launch_row_sumsq(hipStream_t s, const double* X, int64_t N, int d, double* out) {
    if (N <= 0) return 0;
    const unsigned grid = (unsigned)std::min<int64_t>((N + 255) / 256, 4096);
    if (d % 2 == 0 && ((uintptr_t)X & 15) == 0) hipLaunchKernelGGL(row_sumsq_kernel<true>, dim3(grid), dim3(256), 0, s, X, N, d, out);
    else hipLaunchKernelGGL(row_sumsq_kernel<false>, dim3(grid), dim3(256), 0, s, X, N, d, out);
    return kstatus("row_sumsq_kernel");
}

int launch_cos_fix_seg(hipStream_t s, const AssignJob& q, int nlists, const RecList* lists, const double* xn2,
                       const double* nbv) {
    const int nseg = nlists > 0 ? lists[0].nseg : 0;
    if (nseg <= 0) return 0;
    if (nlists > 2) return -1;                       // LSHKM_ERR_ARG
    const Pts X = q.X;
    const int d = q.d, metric = q.metric;
    const double* C = q.C;
    const int32_t* assign = q.assign;
    double* dist = q.dist;
    const int64_t seg_rows = lists[0].seg_rows;
    CosLists cl{};
    for (int i = 0; i < nlists; i++) { cl.list[i] = lists[i].p; cl.counts[i] = lists[i].counts; }
    const dim3 grid((unsigned)(nlists * nseg * CF_SPLIT));
#define CF_LAUNCH(TX, M, XP) hipLaunchKernelGGL((cos_fix_seg_kernel<TX, M>), grid, dim3(256), 0, s, XP, d, C, cl, nseg, seg_rows, assign, dist, xn2, nbv)
    if (metric == 1) {
        if (X.f64) CF_LAUNCH(double, 1, X.d()); else CF_LAUNCH(float, 1, X.f());
    } else {
        if (X.f64) CF_LAUNCH(double, 0, X.d()); else CF_LAUNCH(float, 0, X.f());
    }
#undef CF_LAUNCH
    return kstatus("cos_fix_seg_kernel");
}

}  // namespace lshkm
