// hash_tile.h — the split-f16 MFMA hash tile, one definition
// for the standalone hash (hash_mfma.hip) and the fused pass (fused_hi.hip).
// A wave takes 32 points as the MFMA B operand (lane half h: dims 16s+8h..+7
// of point lane&31) and the 32 projection rows (hi and lo f16 images, LDS) as
// A. A value is certified in f32 against a rigorous window; the others are
// listed and redone from the exact row (hash_exact.h). The kernels keep what
// differs: where the values go, their fences, how they hold the constants.
#pragma once
#include "tile.h"

namespace lshkm {

// The projections' hi / lo f16 images [32][128] into padded LDS rows (FU_RS).
template <int THREADS>
__device__ inline void hash_stage_images(const _Float16* __restrict__ Vh, const _Float16* __restrict__ Vl,
                                         _Float16* lvh, _Float16* lvl) {
    for (int e = threadIdx.x; e < 32 * 16; e += THREADS) {
        const int r = e >> 4, g = e & 15;
        *reinterpret_cast<float4*>(lvh + r * FU_RS + g * 8) = *reinterpret_cast<const float4*>(Vh + r * FU_D + g * 8);
        *reinterpret_cast<float4*>(lvl + r * FU_RS + g * 8) = *reinterpret_cast<const float4*>(Vl + r * FU_D + g * 8);
    }
}

// Window coefficients of one function (pnorm >= |v|_2, v1 >= |v|_1, rounded
// up) for B = |y| G + |x| P + Q (certify_floor_f32). EUCLID: in units of y =
// (acc + t) / w; cosine: of the inner product (t, w unused). FU_A1H is the
// tile's derived sum (tile.h): hash_tile_step's roundings, the callers' seven
// step additions, the split's dropped product and residuals, its margin.
// 1 + 2^-20 covers the roundings of the products here and of f32(1/w),
// 1 + 2^-18 those of B, y -+ B. The fix-up (hash_exact.h) decides a listed
// value from the exact row with its own fp64 bound and reads none of this.
template <bool EUCLID>
__device__ inline void hash_window(double pnorm, double v1, float t, float w, float& P, float& Q) {
    const double iwu = EUCLID ? (double)(1.0f / w) * (1.0 + 0x1p-20) : 1.0;
    const double tf = EUCLID ? fabs((double)t) : 0.0;
    P = (float)((FU_A1H * pnorm * (1.0 + 0x1p-20) + FU_A2 * FU_SQRT_D) * iwu * (1.0 + 0x1p-18));
    Q = (float)((FU_A2 * v1 * (1.0 + 0x1p-20) + (0x1p-40 + 0x1p-23) * tf) * iwu * (1.0 + 0x1p-18) + 0x1p-126);
}

// This lane's 64 values of an fp32 row, B-operand layout: xr = the row + 8 *
// (lane half); dst[8s..8s+7] = dims 16s + 8h .. + 7. 16 loads of 16 B.
__device__ inline void load_row_b(const float* __restrict__ xr, float (&dst)[64]) {
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const float4 p0 = *reinterpret_cast<const float4*>(xr + 16 * s);
        const float4 p1 = *reinterpret_cast<const float4*>(xr + 16 * s + 4);
        dst[8 * s + 0] = p0.x; dst[8 * s + 1] = p0.y; dst[8 * s + 2] = p0.z; dst[8 * s + 3] = p0.w;
        dst[8 * s + 4] = p1.x; dst[8 * s + 5] = p1.y; dst[8 * s + 6] = p1.z; dst[8 * s + 7] = p1.w;
    }
}

// One 16-dim step of a row: hi part of this lane's 8 values (LO: and the lo
// part), |x|^2 (n2a, n2b) and |x - xh|^2 (r2) partial sums.
template <bool LO>
__device__ __forceinline__ void split_norm_step(const float* x8, half8& hi, half8& lo, float2v& n2a, float2v& n2b,
                                                float2v& r2) {
    split8_hi<LO>(x8, hi, lo, r2);
#pragma unroll
    for (int j = 0; j < 8; j += 4) {
        const float2v u = {x8[j], x8[j + 1]}, v = {x8[j + 2], x8[j + 3]};
        n2a = __builtin_elementwise_fma(u, u, n2a);
        n2b = __builtin_elementwise_fma(v, v, n2b);
    }
}

// Step s of the hash tile after the split (bh, bl: hi and lo f16 of this lane's
// 8 values): a fresh accumulator (C = 0), the lo products first, then the hi
// products into it. Each MFMA makes 16 additions, each rounding by at most
// 2^-23 relative and in no assumed order: a hi product passes through 16 of
// them (FU_A1H_MFMA), a lo product through all 48 at 2^-10 of the magnitude
// (FU_A1H_LO). The caller adds the 8 steps with VALU f32 adds, round to
// nearest: 7 more at 2^-24 (FU_A1H_STEPS). A caller that chained the steps
// through the C operand instead would have to charge them at 2^-23.
// vh_row / vl_row: this lane's projection row in the LDS images + 8 * (lane
// half). The packed-f32 step add stays written out in the kernels, and
// hash_mfma_kernel keeps its own row load and split: moved in here they change
// the kernels' register allocation (profiles/README.md).
__device__ __forceinline__ floatx16 hash_tile_step(int s, const _Float16* vh_row, const _Float16* vl_row,
                                                   const half8& bh, const half8& bl) {
    const half8 ah = *reinterpret_cast<const half8*>(vh_row + 16 * s);
    const half8 al = *reinterpret_cast<const half8*>(vl_row + 16 * s);
    const floatx16 z = {};
    floatx16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, z, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}

// Certification in f32 (the floor only needs y to ~2^-20): with
// u = f32(dot~ + t), y = f32(u * f32(1/w)),
//   |y - (x.v + t)/w| <= (Ed + 2^-23 |u| + 2^-40 |t|) / w + 2^-21 |y|,
// Ed = A1 |v||x| + A2 (|v|_1 + |x|_1) + 2^-23 |dot~|: A1 = FU_A1H, the tile's
// bound term by term (tile.h), which charges nothing for a final hi + lo add;
// the 2^-23 |dot~| of the older tile's separate lo accumulator stays in G as
// slack (this tile has no such add), and the reference's x87 / double-product
// roundings are below 2^-50 (|v||x| + |t|). With |x|_1 <= sqrt(d) |x|, |dot~| <=
// |u| + |t| and |u| / w <= |y| (1 + 2^-19), that is at most
//   B = |y| G + |x| P_f + Q_f,   G = (2^-22 + 2^-20)(1 + 2^-18),
//   P_f = (A1 |v| + A2 sqrt(d)) / w,  Q_f = (A2 |v|_1 + (2^-23 + 2^-40)|t|) / w
// (hash_window; the 1 + 2^-18 factors cover the f32 roundings of B, y - B,
// y + B): floor(y - B) == floor(y + B) certifies the reference's floorl.
// nxf >= |x|. v is floor(y - B) in either case. The window is valid for rows
// inside the f16 range only (|x| <= FU_RANGE): the caller lists the others.
__device__ __forceinline__ bool certify_floor_f32(float acc, float t, float iw, float nxf, float P, float Q, int32_t& v) {
    constexpr float G = (0x1p-22f + 0x1p-20f) * (1.f + 0x1p-18f);
    const float y = (acc + t) * iw;
    const float B = fmaf(fabsf(y), G, fmaf(nxf, P, Q));
    const float lo = floorf(y - B), hi = floorf(y + B);
    v = (int32_t)lo;
    return lo == hi;
}
// The same for the four functions of one table (k = 4): certify_floor_f32's
// arithmetic per function, the operations in its order. Returns the table's
// mask, bit q set where function q is NOT certified; the caller shifts it to
// the table's place (one shift per table instead of a 1 << f constant per
// function held in a register).
__device__ __forceinline__ uint32_t certify_floor4_f32(const float* acc4, const float4& t4, float iw, float nxf,
                                                       const float4& P4, const float4& Q4, int32_t (&v)[4]) {
    const float t[4] = {t4.x, t4.y, t4.z, t4.w}, P[4] = {P4.x, P4.y, P4.z, P4.w}, Q[4] = {Q4.x, Q4.y, Q4.z, Q4.w};
    uint32_t bad = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (!certify_floor_f32(acc4[q], t[q], iw, nxf, P[q], Q[q], v[q])) bad |= 1u << q;
    return bad;
}
// CosineHGen: ip >= 0, certified when |acc~| exceeds |x| P_f + Q_f (no t, no w).
__device__ __forceinline__ bool certify_sign_f32(float acc, float nxf, float P, float Q, int& bit) {
    const float B = fmaf(nxf, P, Q);
    bit = acc >= 0.f ? 1 : 0;
    return fabsf(acc) > B;
}

}  // namespace lshkm
