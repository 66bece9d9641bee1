// fused_impl.h — what the fused-pass translation units share: the device
// helpers and sizes used by more than one kernel file, the typed workspace, and
// the host entry of each kernel file (fused.hip's fused_assign calls them in
// sequence).
//   fused_chunked.hip  fused_kernel<HASH>: the streaming form (k != 4; tests)
//   fused_hi.hip       fused_hi_kernel: one f16 MFMA per centroid product
//   fused_refine.hip   fused_persistent_kernel: the 3-product refinement of
//                      the rows a hi-only pass left uncertified
//   fused_small.hip    centroid prep, hash / distance fix-ups, row sums
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "hash_exact.h"
#include "exact.h"
#include "hash_tile.h"
#include "fused_args.h"
#include "pair_merge.h"
#include "pick.h"

namespace lshkm {

// ---- settled launch shapes (the measurements: DESIGN.md, "tried and rejected")
// (the wave counts and centroids per pass that size the workspace: fused_layout.h)
static_assert(FU_D == FUSED_DIMS, "fused_layout.h states the kernels' dimension");
constexpr int FP_THREADS = 64 * FP_WAVES;
constexpr int FH_GATH_KMAX = 256;    // hi-only: the LDS-DMA gather ring fits beside this many centroids
constexpr int FP_HC_BYTES = 32 * (4 + 4 + 4 + 4);     // hash constants |v|_2, |v|_1, t, r
constexpr int MFMA_PRIO = 1;         // s_setprio inside the centroid loop (measured +1-3%)
constexpr int CHAIN_PRIO = 2;        // s_setprio around the hi-only kernel's winner chain (measured -0.02 ms)

// ---- the workspace of one call, typed (fused.hip binds it to the context's
// buffers by fused_layout.h's sizes and regions; null: this shape has none)
struct FusedWorkspace {
    int64_t list_cap = 0;
    _Float16 *Ch = nullptr, *Cl = nullptr;       // [Kpad][128] split-f16 centroid images
    float *cbound = nullptr, *cnh = nullptr;     // FusedArgs::cbound / cnh
    double* nbv = nullptr;                       // [Kpad] sequential |c|^2 (cosine)
    float *C32 = nullptr, *rn32 = nullptr;       // f32(c) [Kpad][128] and |c - f32(c)|_2 [Kpad] rounded up
    double* C64p = nullptr;                      // general rows of d < 128: zero-padded fp64 centroids
    int32_t *list1 = nullptr, *seg1 = nullptr;   // the hi-only passes' rows (seg1: + the hash fix-ups' counts)
    int32_t *list2 = nullptr, *seg2 = nullptr;   // the refinement's rows (seg2: + its declines' counts)
    int32_t* seg3 = nullptr;                     // counts of cfix
    unsigned long long *hfix = nullptr, *cfix = nullptr, *hfix2 = nullptr;   // FusedLayout::fix regions
    unsigned long long* pairs = nullptr;         // ... the refinement's pair rows (counts beside list2's)
    float4* part = nullptr;                      // pass state (Kpad > FP_KMAX)
    unsigned long long* cnt = nullptr;           // CNT_* device counters
    double* xn2 = nullptr;                       // cosine on fp64 rows: [N] sum_j pow(x_j, 2)
    int32_t* tuples = nullptr;                   // hashing without a caller's tuple buffer
};

// ---- host entries of the kernel files. Each picks its instantiation from
// run-time values; a combination no kernel was built for is an error (-1).
// Centroid prep into w (Ch, Cl, cnh, cbound; cosine: nbv; C32 / rn32 and C64p where bound).
int launch_fused_prep(hipStream_t s, const double* C, int K, int d, int metric, const FusedWorkspace& w);
// out[i] = sum_j pow(x_ij, 2) in j order (glibc's pow, gpow2.h), fp64 rows
int launch_row_sumsq(hipStream_t s, const double* X, int64_t N, int d, double* out);
int launch_fused_chunked(hipStream_t s, bool hash, const FusedArgs& a);
// One hi-only pass over all rows; a.Kpad centroids from a.Ch / a.cnh.
struct HiForm {
    bool hash = false;       // hash tile + LSH outputs in this pass
    bool mp = false;         // one of several passes (a.t0 / a.pass_first / a.pass_last)
    int metric = 0;          // 1: cosine
    bool two_image = false;  // 512 < Kpad <= 1024 in one launch
    bool gath = false;       // winner rows through the LDS-DMA gather ring
    int rows = 0;            // 0: fp32 d = 128, 1: fp32 d <= 128, 2: fp64 d <= 128
    bool fast = false;       // the certified f32 winner distance compiled in
    bool rowpf = false;      // the next tile's rows fetched one tile ahead (fast, one pass, fp32 d = 128)
};
int launch_fused_hi_pass(hipStream_t s, unsigned nblk, const HiForm& f, FusedArgs a);
// One refinement pass over the rows of a.list_in; a.Kpad <= FP_KMAX centroids.
int launch_fused_refine_pass(hipStream_t s, unsigned nblk, int metric, bool mp, int rows, const FusedArgs& a);
// Fix-up of the hash values listed in l (a: the pass's block; its list fields are set from l).
void launch_hash_fixup(hipStream_t s, const RecList& l, bool cosine, FusedArgs a);
// Winners listed by the fused kernels for their distance alone (nlists <= 2
// segmented lists of one grid): metric 1 the soft-x87 cosine, metric 0 the
// euclidean chain with glibc's pow(x, 2) (gpow2.h).
int launch_cos_fix_seg(hipStream_t s, const AssignJob& q, int nlists, const RecList* lists, const double* xn2,
                       const double* nbv);

// Profiling builds (make prof -> liblshkm_prof.so) accumulate s_memtime per
// phase of the persistent loop; the product library compiles these away.
#ifdef LSHKM_PHASE_TIMING
#define PT_DECL unsigned long long pt_acc[6] = {0, 0, 0, 0, 0, 0}; unsigned long long pt_t = __builtin_amdgcn_s_memtime();
#define PT_MARK(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); pt_acc[i] += t_ - pt_t; pt_t = t_; }
#define PT_FLUSH if (lane == 0) for (int i_ = 0; i_ < 6; i_++) atomicAdd(a.prof + i_, pt_acc[i_]);
#elif defined(LSHKM_ISA_MARK)       // assembly listings: region comments (tools/isa_regions.py)
#define PT_DECL
#define PT_MARK(i) asm volatile(";PTMARK " #i);
#define PT_FLUSH
#else
#define PT_DECL
#define PT_MARK(i)
#define PT_FLUSH
#endif

// __shfl_xor(v, 32) as two v_permlane32_swap (gfx950 VALU lane-half swap)
// instead of two LDS bpermutes: sw[0] holds the lower half's value in the
// upper lanes, sw[1] the upper half's value in the lower lanes.
__device__ inline double swap_halves(double v, int h) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)b, (uint32_t)b, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)(b >> 32), (uint32_t)(b >> 32), false, false);
    const uint32_t l = h ? lo[0] : lo[1], u = h ? hi[0] : hi[1];
    return __longlong_as_double((long long)(((uint64_t)u << 32) | l));
}

__device__ inline float swap_halves_f(float v, int h) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(h ? r[0] : r[1]);
}

// One direction of the half swap (the chain hand-offs): take_from_lower gives
// the upper lanes the lower half's value and leaves the lower lanes' own (the
// first result of v_permlane32_swap(v, v)); take_from_upper the other way.
// No select: one v_permlane32_swap per dword.
__device__ inline double take_from_lower(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t l = __builtin_amdgcn_permlane32_swap((uint32_t)b, (uint32_t)b, false, false)[0];
    const uint32_t u = __builtin_amdgcn_permlane32_swap((uint32_t)(b >> 32), (uint32_t)(b >> 32), false, false)[0];
    return __longlong_as_double((long long)(((uint64_t)u << 32) | l));
}
__device__ inline double take_from_upper(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t l = __builtin_amdgcn_permlane32_swap((uint32_t)b, (uint32_t)b, false, false)[1];
    const uint32_t u = __builtin_amdgcn_permlane32_swap((uint32_t)(b >> 32), (uint32_t)(b >> 32), false, false)[1];
    return __longlong_as_double((long long)(((uint64_t)u << 32) | l));
}

// One 32-row tile: acc_hi = sum(Ah Bh), acc_lo = sum(Ah Bl + Al Bh).
__device__ inline void tile_mfma(const _Float16* ah_row, const _Float16* al_row, const half8 (&bh)[8],
                                 const half8 (&bl)[8], floatx16& acc_hi, floatx16& acc_lo) {
#pragma unroll
    for (int r = 0; r < 16; r++) { acc_hi[r] = 0.f; acc_lo[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const half8 ah = *reinterpret_cast<const half8*>(ah_row + 16 * s);
        const half8 al = *reinterpret_cast<const half8*>(al_row + 16 * s);
        acc_hi = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[s], acc_hi, 0, 0, 0);
        acc_lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[s], acc_lo, 0, 0, 0);
        acc_lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[s], acc_lo, 0, 0, 0);
    }
}

// General rows (ROWS = 1: fp32, 2: fp64; d <= 128 dims, row stride d): lane
// half h's 64 values of row rowc in the B-operand layout (dims 16s+8h..+7),
// zero past d; fp64 values rounded to f32 (the scores' operand; the bounds add
// |x - f32(x)| <= 2^-24 |x|).
template <int ROWS>
__device__ inline void load_row_gen(const FusedArgs& a, int64_t rowc, int h, float (&dst)[64]) {
    const int64_t ro = rowc * (int64_t)a.d;
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const int j0 = 16 * s + 8 * h;
        if (a.xvec && j0 + 8 <= a.d) {
            if constexpr (ROWS == 1) {
                const float4 p0 = *reinterpret_cast<const float4*>(a.X + ro + j0);
                const float4 p1 = *reinterpret_cast<const float4*>(a.X + ro + j0 + 4);
                dst[8 * s + 0] = p0.x; dst[8 * s + 1] = p0.y; dst[8 * s + 2] = p0.z; dst[8 * s + 3] = p0.w;
                dst[8 * s + 4] = p1.x; dst[8 * s + 5] = p1.y; dst[8 * s + 6] = p1.z; dst[8 * s + 7] = p1.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double2 q = *reinterpret_cast<const double2*>(a.X64 + ro + j0 + 2 * j);
                    dst[8 * s + 2 * j] = (float)q.x;
                    dst[8 * s + 2 * j + 1] = (float)q.y;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float v = 0.f;
                if (j0 + e < a.d) v = ROWS == 1 ? a.X[ro + j0 + e] : (float)a.X64[ro + j0 + e];
                dst[8 * s + e] = v;
            }
        }
    }
}
// fp64 rows: the exact values of 16-dim step st of lane half h (the winner chain)
__device__ inline void load_x64_step(const FusedArgs& a, int64_t rowc, int st, int h, double2 (&o)[4]) {
    const int64_t ro = rowc * (int64_t)a.d;
    const int j0 = 16 * st + 8 * h;
    if (a.xvec && j0 + 8 <= a.d) {
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = *reinterpret_cast<const double2*>(a.X64 + ro + j0 + 2 * j);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            o[j] = make_double2(0.0, 0.0);
            if (j0 + 2 * j < a.d) o[j].x = a.X64[ro + j0 + 2 * j];
            if (j0 + 2 * j + 1 < a.d) o[j].y = a.X64[ro + j0 + 2 * j + 1];
        }
    }
}

// Running best / runner-up over one tile's scores. Each score carries its
// in-tile index (4g+q) in its low 4 mantissa bits (see E), so the best needs
// no compare/select per score. Per pair (ta, tb) of new scores:
//   m2 = max(m2, med3(m1, ta, tb)),  m1 = max3(m1, ta, tb)
// (the runner-up of {m1 >= m2, ta, tb} is the larger of m2 and the median of
// the other three): 3 VALU per 2 scores. v_max3 / v_med3 as instructions:
// fmaxf would first re-quiet its operands (IEEE mode); scores are finite for
// any certifiable point.
__device__ inline float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ inline void tile_epilogue(const float (&sv)[16], float& m1, float& m2) {
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const float ta = __uint_as_float((__float_as_uint(sv[r]) & ~0xFu) | (uint32_t)r);
        const float tb = __uint_as_float((__float_as_uint(sv[r + 1]) & ~0xFu) | (uint32_t)(r + 1));
        m2 = __builtin_amdgcn_fmed3f(m2, __builtin_amdgcn_fmed3f(m1, ta, tb), 0x1.fffffep127f);
        m1 = vmax3(m1, ta, tb);
    }
}

// The refinement's epilogue where it names the runner-up too (pair_merge.h):
// the tile's own best three first -- its 16 scores differ in their index bits,
// so they are distinct and three med3 / max steps per score keep them sorted --
// then those three, best first, into the running state with the tile's number.
// m1 and m2 take the values tile_epilogue gives them, and t1 the tile it notes.
__device__ inline void tile_epilogue3(const float (&sv)[16], int tile, Top3& s) {
    float a1 = -__builtin_inff(), a2 = a1, a3 = a1;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float v = __uint_as_float((__float_as_uint(sv[r]) & ~0xFu) | (uint32_t)r);
        a3 = __builtin_amdgcn_fmed3f(a3, a2, v);
        a2 = __builtin_amdgcn_fmed3f(a2, a1, v);
        a1 = vmax3(a1, v, v);
    }
    top3_insert(s, a1, tile);
    top3_insert(s, a2, tile);
    top3_insert(s, a3, tile);
}

}  // namespace lshkm
