// tile.h — the split-f16 MFMA tile helpers shared by the fused hash+assign
// pass (fused.hip) and the standalone MFMA hash (hash_mfma.hip; the hash tile
// itself: hash_tile.h): operand types, the certification constants of DESIGN.md
// §4, EuclideanPhi's 32-bit arithmetic (euclidean_phi_gen.hpp:70-92) and the
// bucket division.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lshkm {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int FU_D = 128;                // dimension handled by this kernel
constexpr int FU_RS = FU_D + 8;          // f16 LDS row stride (elements) = 272 B

// The split-f16 dot product's error (DESIGN.md §4 "Split-f16 scores"):
//   |dot~ - x.v| <= A1 |x||v| + A2 (|x|_1 + |v|_1),
// A1 a sum of named parts, each relative to sum_j |x_j v_j| <= |x||v|
// (Cauchy-Schwarz). The one assumption about the MFMA: every addition inside it
// rounds somehow, by at most 2^-23 relative (FU_U_ANY; nothing about its order).
// A term that passes through n such additions carries at most n * 2^-23 of its
// magnitude (second order: FU_MARGIN). What the users add themselves is not in
// A1: the 3-product forms' final hi + lo add, the hash's + t and * (1/w)
// (certify_floor_f32's G), the scores' + cn.
constexpr double FU_U_ANY = 0x1p-23;     // one addition, any rounding mode or MFMA-internal
constexpr double FU_U_RN = 0x1p-24;      // one VALU f32 addition, round to nearest (no kernel sets the mode)
// x = xh + xl + r, xh = f16(x), xl = f16(x - xh), |r| <= 2^-22 |x| in the f16
// normal range (subnormal lo parts: A2); the same for v. x.v - (xh.vh + xh.vl +
// xl.vh) = xl.vl + r_x.v + (xh + xl).r_v:
constexpr double FU_SPLIT_DROPPED = 0x1p-22;        // the product xl.vl, never formed
constexpr double FU_SPLIT_RESID = 2 * 0x1p-22;      // r_x.v and (xh + xl).r_v
// sum |lo products| = sum |xh vl| + |xl vh| <= 2 * 2^-11 sum |x v|
constexpr double FU_LO_SHARE = 0x1p-10;
// Safety factor on the sum, 1 + 2^-8 (3.9 parts in a thousand) for what the
// parts leave out: |xh| <= (1 + 2^-11)|x| and the same for v and the lo parts
// (< 1 + 2^-9 together), (1 + u)^n - 1 against n u (n <= 256: < 1 + 2^-15), a
// round-up's error measured on its result instead of the exact sum (1 + 2^-23),
// fp64 projections whose lo part is rounded to f32 first (1 + 2^-13), the
// reference's own x87 / double-product roundings (2^-50 |x||v|). pnorm and
// v1 are rounded up where they are formed and need none of it.
constexpr double FU_MARGIN = 1.0 + 0x1p-8;

// 3-product tile (tile_mfma, fused_impl.h): acc_hi chains the 8 steps' hi
// products through the MFMA's C operand, acc_lo the 16 lo MFMAs.
constexpr double FU_A1_HI_CHAIN = 128 * FU_U_ANY;              // 8 MFMAs x 16 additions in one chain
constexpr double FU_A1_LO_CHAIN = 256 * FU_U_ANY * FU_LO_SHARE;   // 16 MFMAs x 16, on the lo products
constexpr double FU_A1_C_F32 = FU_U_RN;             // centroids: c rounded to f32 before its split (fused_centroid_prep)
constexpr double FU_A1 = (FU_A1_HI_CHAIN + FU_A1_LO_CHAIN + FU_A1_C_F32 + FU_SPLIT_DROPPED + FU_SPLIT_RESID) * FU_MARGIN;
// = 1.0568 * 2^-16

// Hash tile (hash_tile_step, hash_tile.h; every hashing form of fused_hi.hip
// and hash_mfma.hip): each 16-dim step starts a fresh accumulator (C = 0), the
// two lo MFMAs first, the hi MFMA last; the caller adds the 8 steps with VALU
// packed-f32 adds (v_pk_add_f32, round to nearest). A form that chained the
// steps through the MFMA's C operand would need FU_U_ANY for them, or FU_A1.
constexpr double FU_A1H_MFMA = 16 * FU_U_ANY;       // a hi product: the 16 additions of the step's last MFMA
constexpr double FU_A1H_LO = 48 * FU_U_ANY * FU_LO_SHARE;    // a lo product: all 3 x 16 additions of its step
constexpr double FU_A1H_STEPS = 7 * FU_U_RN;        // the 7 step additions, VALU
constexpr double FU_A1H = (FU_A1H_MFMA + FU_A1H_LO + FU_A1H_STEPS + FU_SPLIT_DROPPED + FU_SPLIT_RESID) * FU_MARGIN;
// = 0.8015 * 2^-18
constexpr double FU_A2 = 0x1p-24;
constexpr float FU_RANGE = 32768.f;

// phi % nb by multiply-high (Granlund-Montgomery round-up, 31-bit numerators):
// nb in [2, 2^31), l = ceil(log2 nb), m = floor(2^(31+l) / nb) + 1 < 2^32,
// q = (m * phi) >> (31 + l). nb == 1 -> 0; nb >= 2^31 -> phi (phi < 2^31).
struct BucketDiv {
    uint32_t m, nb;
    int sh, mode;           // mode 0: magic, 1: nb == 1, 2: nb > phi always
};
__host__ inline BucketDiv make_bucket_div(int64_t nb) {
    BucketDiv b{0u, 0u, 0, 0};
    if (nb <= 1) { b.mode = 1; return b; }
    if (nb >= (1ll << 31)) { b.mode = 2; return b; }
    int l = 0;
    while ((1ll << l) < nb) l++;
    b.m = (uint32_t)((((unsigned __int128)1 << (31 + l)) / (unsigned __int128)nb) + 1);
    b.nb = (uint32_t)nb;
    b.sh = l - 1;
    return b;
}

typedef float float2v __attribute__((ext_vector_type(2)));
constexpr double FU_SQRT_D = 11.313708498984761 * (1.0 + 0x1p-40);   // sqrt(128), rounded up

typedef _Float16 half2v __attribute__((ext_vector_type(2)));
// x - f32(h) in one v_fma_mix_f32 (x * 1 - h, the f16 operand widened exactly,
// one rounding: the same value as x - (float)h), h the low / high half of hp.
__device__ inline float resid_lo(float x, half2v hp) {
    float r;
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x), "v"(hp));
    return r;
}
__device__ inline float resid_hi(float x, half2v hp) {
    float r;
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x), "v"(hp));
    return r;
}

// EuclideanPhi arithmetic (euclidean_phi_gen.hpp:70-92) in 32-bit form, M =
// int(pow(2,32)-5) = 2^31-1 under g++. temp = (long)(h * r) is an int32 (the
// int product wraps), so ((temp % M) + M) % M needs only compares; the uint32
// sum hn wraps, and (hn % M + M) % M = hn % M for hn < 2^32.
constexpr uint32_t PHI_M = 2147483647u;
__device__ inline uint32_t phi_term(int32_t h, int32_t r) {
    int64_t v = (int32_t)((uint32_t)h * (uint32_t)r);    // in [-2^31, 2^31)
    if (v >= (int64_t)PHI_M) v -= PHI_M;
    if (v < 0) v += PHI_M;
    if (v < 0) v += PHI_M;                                 // only v = -2^31
    return (uint32_t)v;
}
__device__ inline uint32_t phi_final(uint32_t hn) {
    if (hn >= PHI_M) hn -= PHI_M;
    if (hn >= PHI_M) hn -= PHI_M;
    return hn;
}
// Certified hashes have |h| < 2^22 and r in [0, 100] (euclidean_phi_gen.hpp:64;
// ProjTable::r_small), so h * r does not wrap, both operands fit 24 bits (one
// full-rate v_mul_i32_i24 instead of a quarter-rate v_mul_lo_u32) and
// ((temp % M) + M) % M is one select. Uncertified h are rewritten by the fix-up.
__device__ inline uint32_t phi_term_small(int32_t h, int32_t r) {
    const int32_t p = __mul24(h, r);
    return p < 0 ? (uint32_t)p + PHI_M : (uint32_t)p;
}
// The uint32 sum of a table's four phi_term_small terms without a select per
// term. With s = p >> 31 (arithmetic: -1 or 0), p + (p < 0 ? M : 0) = p - M s
// for every int32 p, so the wrapping sum of the four terms is
//   (p0 + p1 + p2 + p3) - M (s0 + s1 + s2 + s3)   (mod 2^32),
// the same ring element, and M x = (x << 31) - x. Same contract as
// phi_term_small (|h| < 2^22, r in [0, 100], M = 2^31 - 1) for the products;
// the identity itself holds for any p, so uncertified h give the same
// (rewritten) value as the term-by-term form too.
__device__ inline uint32_t phi_sum4_small(const int32_t (&h)[4], const int32_t (&r)[4]) {
    const int32_t p0 = __mul24(h[0], r[0]), p1 = __mul24(h[1], r[1]), p2 = __mul24(h[2], r[2]), p3 = __mul24(h[3], r[3]);
    const uint32_t sp = (uint32_t)p0 + (uint32_t)p1 + (uint32_t)p2 + (uint32_t)p3;
    const uint32_t ss = (uint32_t)((p0 >> 31) + (p1 >> 31) + (p2 >> 31) + (p3 >> 31));
    return sp + ss - (ss << 31);
}
__device__ inline int32_t bucket_fast(uint32_t ph, const BucketDiv& b) {
    if (b.mode == 1) return 0;
    if (b.mode == 2) return (int32_t)ph;
    const uint32_t q = __umulhi(ph, b.m) >> b.sh;
    return (int32_t)(ph - q * b.nb);
}

// hi = f16(x) of 8 values; r = x - f32(hi) (one v_fma_mix each, exact) summed
// as r^2 into r2; LO: lo = f16(r) as well (the 3-product hash tile).
template <bool LO>
__device__ inline void split8_hi(const float* x, half8& hi, half8& lo, float2v& r2) {
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const half2v hp = {(_Float16)x[j], (_Float16)x[j + 1]};
        hi[j] = hp.x;
        hi[j + 1] = hp.y;
        const float2v r = {resid_lo(x[j], hp), resid_hi(x[j + 1], hp)};
        r2 = __builtin_elementwise_fma(r, r, r2);
        if (LO) {
            lo[j] = (_Float16)r.x;
            lo[j + 1] = (_Float16)r.y;
        }
    }
}

}  // namespace lshkm
