// fused_hi.hip — the hi-only form of the fused pass (fused.hip).
// Lloyd (+ hashing, euclidean) with ONE f16 MFMA per centroid product: the
// score is t~ = acc(-|c|^2/2 + sum_j xh_j ch_j), the accumulator initialised
// with the f32 -|c|^2/2 (no epilogue add), ch = f16(f32(c)), xh = f16(x);
// cosine (MET = 1): the normalised centroid rows, no offset.
// Bound (rigorous, |x_j| <= 2^15, c in range): with xr = x - xh (exact in f32)
// and cr = c - ch,
//   |t~ - t| <= |xh||cr| + |xr||c| + 2^-24|cn| + A (|cn| + |xh||ch|),
//   A = 130 2^-23 (<= 129 round-toward-zero additions of partial sums bounded
//   by |cn| + sum|xh_j ch_j|), plus the terms of the 3-product form for the
//   reference's own fp64 roundings (2^-41 (|x|^2 + |c|^2)) and the packed tile
//   index (2^-18 (|x||c| + |cn|)); |xr| is summed per row, the centroid
//   maxima come from the prep (cbound[3..6]). A point is certified iff
//   M2 < M1 - 2E; the others (~3% of N(0,1) rows at K = 256) are listed for the
//   3-product form (fused_persistent_kernel, fused_refine.hip), which certifies
//   all but ~1% of those and lists the rest for the exact pass.
// One third of the MFMA work of the 3-product form, and only the hi image of
// the centroids in LDS: up to 512 centroids per pass (K = 1024: 2 passes).
#include "fused_impl.h"

namespace lshkm {

__host__ __device__ constexpr int fh_lds_bytes(int Kpad, bool hash) {
    return 16 + Kpad * FU_RS * 2 + Kpad * 4 + (hash ? 2 * 32 * FU_RS * 2 + FP_HC_BYTES : 0);
}
static_assert(fh_lds_bytes(FH_KMAX, true) <= 160 * 1024, "hi-only LDS image exceeds 160 KiB");
constexpr double FH_A = 130.0 * 0x1p-23;

// Waves per block of the hi-only form (one block per CU), per instantiation:
// 8 unless a third wave per SIMD fits without spills and pays (the 8- vs
// 12-wave measurements: DESIGN.md, "tried and rejected").
constexpr int FH_WAVES_MPFAST = 12;  // the last pass of the multi-pass form with the certified distance
constexpr int FH_FAST_WAVES = 8;     // the single-pass FAST form (the headline kernel)
template <bool HASH, bool MP, int MET, bool FAST = false>
__host__ __device__ constexpr int fh_waves() {
    return HASH && MP ? 12 : (MP && FAST ? FH_WAVES_MPFAST : (FAST && !MP ? FH_FAST_WAVES : 8));
}

// The upper half's finish of the cosine winner certificate (IpAcc, exact.h):
// the halves' double-double sums joined by one TwoSum; sum_k |S_k| bound
// rounded up (+ 2^-47 relative for the roundings of |A_k + B_end| and of the
// sums here; the partial sums stand in for the exact ones: their TwoSum rests,
// |sl| <= 64 2^-53 max|t| per half, and the offsets, <= 2^-38 max|t|, charged
// absolutely -- a cancelling A_k + B_end must not hide them). max |t| of both
// halves' running sums <= sum_j |p_j| <= (1 + 2^-53) |x| |c| (Cauchy-Schwarz):
// mb = 2 sqrt(xa nbv) (1 + 2^-40) bounds the pair of them without a per-term
// max; sum |S_k| >= 2^-790 stands in for quot_status's lower range check on
// the partial sums themselves (max |S_k| >= that / 128).
__device__ inline int cosine_halves_finish(double sh0, double sl0, double ts0, double sh, double sl, double ts,
                                           double xa, double nbv, double& v) {
    const double mb = 2.0 * sqrt(__dmul_rn(xa, nbv)) * (1.0 + 0x1p-40);
    const double tsum = __dadd_rn(ts0, ts);
    if (!(tsum >= 0x1p-790)) return 2;
    IpAcc ip;
    const double t = __dadd_rn(sh0, sh);
    const double bb = __dsub_rn(t, sh0);
    const double e = __dadd_rn(__dsub_rn(sh0, __dsub_rn(t, bb)), __dsub_rn(sh, bb));
    ip.sh = t;
    ip.sl = __dadd_rn(__dadd_rn(sl0, sl), e);
    ip.ts = __dadd_rn(tsum * (1.0 + 0x1p-47), 0x1p-37 * mb);
    ip.mx = mb;
    double q, qr;
    const int st = ip.quot_status(__dmul_rn(sqrt(xa), sqrt(nbv)), q, qr);
    if (st == 0) v = __dsub_rn(1.0, q);
    return st;
}

// MET = 1: cosine (the prep's normalised centroid rows, score x.c^ with no
// offset; the winner's distance from the row in registers, declines to the
// cfix list). HASH with MET = 1: CosineHGen signs of the L*k projections
// (k = 4: table l = 2g + h in D registers 4g..4g+3), certified as in
// hash_mfma.hip, g = phi = bucket; uncertified signs to the hfix list.
// Cosine winner distance from the row in registers, both lane halves busy.
// Lane half h owns dims 16s + 8h..+7 (s = 0..7). Each half accumulates the
// double products of ITS dims with IpAcc's double-double (exact.h), in its own
// order; the reference's x87 chain runs over all 128 in order (block 2s = half
// 0's step s, block 2s + 1 = half 1's), so its partial sums are S_k = A_k +
// B_end(s-1) in half 0's block s and S_k = B_k + A_end(s) in half 1's. The
// halves trade their running sums after every step: half 0 adds |A_k + B_end(s-1)|
// exactly as the reference's partial sum, half 1 |B_k + A_end(s-1)| plus
// 8 |A_end(s) - A_end(s-1)| (the block it runs one step behind) -- the round-4
// bound 8 (sum |A_end| + sum |B_end|) roughly doubled sum_k |S_k| and declined
// 9.3 % of the C3 winners. max |S_k| from the norms (cosine_halves_finish;
// exact.h quot_status decides). |x|^2 is the reference's sequential chain, the
// halves taking turns (the euclidean winner's pattern).
// Returns 0 (certified, v = 1 - q), 1 / 2 (declined: soft-x87 fix-up).
__device__ inline int cosine_winner_halves(const float (&xf)[64], const double* __restrict__ crow_h, double nbv, int h,
                                           double& v) {
    // |x|^2: the reference's sequential fp64 chain (cust_vector.hpp:139-155), halves alternating
    double xa = 0.0;
#pragma unroll
    for (int s = 0; s < 8; s++) {
        if (h == 0) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const double xj = (double)xf[8 * s + j];
                xa = __dadd_rn(xa, __dmul_rn(xj, xj));
            }
        }
        xa = take_from_lower(xa);
        if (h == 1) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const double xj = (double)xf[8 * s + j];
                xa = __dadd_rn(xa, __dmul_rn(xj, xj));
            }
        }
        xa = take_from_upper(xa);
    }
    // the inner product, each half over its own dims
    double sh = 0.0, sl = 0.0, ts = 0.0;
    double off = 0.0;                     // half 0: B_end(s-1); half 1: A_end(s-1)
    double2 cb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) cb[j] = *reinterpret_cast<const double2*>(crow_h + 2 * j);
#pragma unroll
    for (int s = 0; s < 8; s++) {
        double cv[8];
#pragma unroll
        for (int j = 0; j < 4; j++) { cv[2 * j] = cb[j].x; cv[2 * j + 1] = cb[j].y; }
        if (s + 1 < 8) {
#pragma unroll
            for (int j = 0; j < 4; j++) cb[j] = *reinterpret_cast<const double2*>(crow_h + 16 * (s + 1) + 2 * j);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const double pj = __dmul_rn((double)xf[8 * s + j], cv[j]);
            const double t = __dadd_rn(sh, pj);
            const double bb = __dsub_rn(t, sh);
            const double e = __dadd_rn(__dsub_rn(sh, __dsub_rn(t, bb)), __dsub_rn(pj, bb));   // TwoSum
            sh = t;
            sl = __dadd_rn(sl, e);
            ts = __dadd_rn(ts, fabs(__dadd_rn(t, off)));
        }
        // trade the running sums: half 0 takes B_end(s), half 1 A_end(s) (and
        // charges the block it ran behind: 8 |A_end(s) - A_end(s-1)|)
        const double other = swap_halves(sh, h);
        if (h == 1) ts = __dadd_rn(ts, 8.0 * fabs(__dsub_rn(other, off)));
        off = other;
    }
    // the lower half's accumulator to the upper lanes
    const double sh0 = swap_halves(sh, h), sl0 = swap_halves(sl, h), ts0 = swap_halves(ts, h);
    if (h == 0) return 2;                 // the upper lanes finish
    return cosine_halves_finish(sh0, sl0, ts0, sh, sl, ts, xa, nbv, v);
}

// The same for fp64 rows (ROWS = 2): the exact x values re-read from the row
// (L2) two 16-dim steps ahead (a rolled loop: unrolled, the loads of all steps
// were hoisted and spilled) for the halves' inner products. Dims past d are
// zero in the row (load_x64_step) and in the padded centroid copy: exact zero
// terms. |x|^2 of a general double row needs glibc's pow(x, 2) per term
// (gpow2.h): the row's sequential sum comes precomputed (a.xn2, row_sumsq).
__device__ inline int cosine_winner_halves_x64(const FusedArgs& a, int64_t rowc, const double* __restrict__ crow_h,
                                               double nbv, int h, double& v) {
    double2 xn[4], xnn[4];
    load_x64_step(a, rowc, 0, h, xn);
    load_x64_step(a, rowc, 1, h, xnn);
    double sh = 0.0, sl = 0.0, ts = 0.0;
    double off = 0.0;                     // as cosine_winner_halves
    double2 cb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) cb[j] = *reinterpret_cast<const double2*>(crow_h + 2 * j);
#pragma unroll 1
    for (int s = 0; s < 8; s++) {
        double xv[8], cv[8];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            xv[2 * j] = xn[j].x; xv[2 * j + 1] = xn[j].y;
            cv[2 * j] = cb[j].x; cv[2 * j + 1] = cb[j].y;
            xn[j] = xnn[j];
        }
        if (s + 2 < 8) load_x64_step(a, rowc, s + 2, h, xnn);
        if (s + 1 < 8) {
#pragma unroll
            for (int j = 0; j < 4; j++) cb[j] = *reinterpret_cast<const double2*>(crow_h + 16 * (s + 1) + 2 * j);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const double pj = __dmul_rn(xv[j], cv[j]);
            const double t = __dadd_rn(sh, pj);
            const double bb = __dsub_rn(t, sh);
            const double e = __dadd_rn(__dsub_rn(sh, __dsub_rn(t, bb)), __dsub_rn(pj, bb));   // TwoSum
            sh = t;
            sl = __dadd_rn(sl, e);
            ts = __dadd_rn(ts, fabs(__dadd_rn(t, off)));
        }
        const double other = swap_halves(sh, h);
        if (h == 1) ts = __dadd_rn(ts, 8.0 * fabs(__dsub_rn(other, off)));
        off = other;
    }
    const double sh0 = swap_halves(sh, h), sl0 = swap_halves(sl, h), ts0 = swap_halves(ts, h);
    if (h == 0) return 2;
    return cosine_halves_finish(sh0, sl0, ts0, sh, sl, ts, a.xn2[rowc], nbv, v);
}

// NIMG = 2 (512 < K <= 1024, euclidean): ONE launch for all centroids. The
// LDS holds one 512-centroid image at a time; the block's waves each score
// their tile against the image in LDS, the block swaps in the other image
// (two barriers, 128 KB from L2), and the waves finish the same tile against
// it with the row still in registers -- no second read of X and no carried
// pass state. Images alternate A,B / B,A between rounds (one swap per round);
// every wave runs the block's round count (tiles past the end: no valid rows).
// GATH (euclidean, one pass, Kpad <= FH_GATH_KMAX): the winner rows of the
// distance chain are gathered into a per-wave LDS ring by LDS-DMA, 8 lanes per
// 128-B row segment (coalesced), instead of 16-B register loads from 32
// different rows per instruction -- the vector-memory path (TA/TD/TCP) was the
// busiest unit of the pass (TD 97 %, TA 88 % busy; 63 % of the L1 accesses
// were these loads). Ring of two 4-KiB steps (16 dims x 32 points x 8 B).
constexpr int FH_GATH_STEP = 32 * 16 * 8;
constexpr int FH_GATH_WAVE = 2 * FH_GATH_STEP;
__host__ __device__ constexpr int fh_gath_off(int Kpad, bool hash) { return (fh_lds_bytes(Kpad, hash) + 255) & ~255; }
static_assert(fh_gath_off(FH_GATH_KMAX, true) + 8 * FH_GATH_WAVE <= 160 * 1024, "gather ring exceeds 160 KiB");

// One LDS-DMA piece: each lane's 16 B at gsrc land at lds_dst + 16 * lane
// (M0 written and restored in the same statement; the load is invisible to the
// compiler's wait counting: the chain waits for it with an explicit vmcnt).
__device__ inline void glds16(const void* gsrc, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// Row prefetch (PF, the FAST single-pass form on fp32 rows of 128 dims): a
// software pipeline one tile deep, per wave, with no barrier. Bit 1 (LDS half):
// dims 0..63 of the next tile's 32 rows by LDS-DMA into the wave's own 8-KiB
// buffer after the image (8 pieces of 1 KiB, four 256-B half rows each); the
// tile's top reads xf[0..31] from it by ds_read_b128. Bit 0 (register half):
// dims 64..127 by 16-B register loads into 32 registers the hash phase has left
// free (the centroid loop needs bh, the accumulator and xf), read in place by
// the next tile (the tile-pair loop: two such sets trade places). Both are
// issued between the hash phase and the centroid tiles (pf_next); either alone
// still waits for the other half at the top (measurement variants,
// -DLSHKM_ROWPF=1 / 2). DESIGN.md §4 has the ordering rules. Row p of the
// buffer holds its 16-B chunk c at position c ^ (p & 15): the 16 rows of a
// ds_read_b128 group on 16 distinct 4-bank groups; the DMA's destination is
// lane-linear, so the swizzle sits on the per-lane source address (as the
// gather ring's).
#ifndef LSHKM_ROWPF
#define LSHKM_ROWPF 3
#endif
constexpr int FH_ROWPF = LSHKM_ROWPF;             // the form the library runs: 0 none, 1 register half, 2 LDS half, 3 both
constexpr int FH_ROWPF_KMAX = 256;                // the FAST single-pass form's largest Kpad
constexpr int FH_ROWPF_WAVE = 32 * 64 * 4;        // 32 rows x 64 dims x 4 B
__host__ __device__ constexpr int fh_rowpf_off(int Kpad, bool hash) { return (fh_lds_bytes(Kpad, hash) + 255) & ~255; }
static_assert(fh_rowpf_off(FH_ROWPF_KMAX, true) + FH_FAST_WAVES * FH_ROWPF_WAVE <= 160 * 1024,
              "row prefetch buffers exceed 160 KiB");
static_assert(FH_ROWPF_KMAX <= FH_GATH_KMAX, "the FAST single-pass form runs where the gather ring would (fused.hip)");

// The same from a scalar base: each lane's 16 B at sbase + voff (an unsigned
// 32-bit byte offset) land at lds_base + lds_off + 16 * lane. lds_off is an
// immediate added into M0 here: eight hoisted base + offset values, one per
// piece, cost eight scalar registers across the whole loop.
__device__ inline void glds16s(const void* sbase, uint32_t voff, uint32_t lds_base, int lds_off) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_add_u32 m0, %3, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_base), "n"(lds_off) : "memory", "scc");
}

// ROWS = 0: fp32 rows of 128 dims (X); 1: fp32 rows of d <= 128 dims; 2: fp64
// rows of d <= 128 dims (X64) -- euclidean Lloyd without hashing, one pass.
// Dims d..127 are zero in the row and in the centroid images (the prep pads
// them). fp64 rows: the scores use xh = f16(f32(x)); |x - f32(x)| <= 2^-24 |x|
// joins |xr| in the bound; the winner chain re-reads the fp64 row (the
// register copy is f32).
// FAST (euclidean, fp32 rows; the last pass when K > 512): the certified f32 winner distance
// compiled in (no fp64 chain state). Its f32 centroid rows are register loads:
// through the gather ring (GATH) each 16-dim step waits on its DMA, and the
// short f32 sum cannot hide that (fused pass 2.21 vs 2.14 ms at C3).
// HG: the hash tile's live groups of four accumulator registers. Group g holds
// tables 2g and 2g + 1; with L <= 2 HG tables the registers past 4 HG hold only
// the zero padding rows of the projection image, and neither their step adds
// nor their certificates are compiled (the launch picks HG from L).
template <bool HASH, bool MP = false, int MET = 0, int NIMG = 1, bool GATH = false, int ROWS = 0, bool FAST = false,
          int PF = 0, int HG = 4>
__global__ __launch_bounds__((64 * fh_waves<HASH, MP, MET, FAST>()), 1) void fused_hi_kernel(FusedArgs a) {
    constexpr int FH_WAVES = fh_waves<HASH, MP, MET, FAST>();
    constexpr int FH_THREADS = 64 * FH_WAVES;
    static_assert(NIMG == 1 || (!MP && MET == 0), "two-image form: euclidean, single launch");
    static_assert(!GATH || (!MP && MET == 0 && NIMG == 1 && FH_WAVES == 8), "gather ring: euclidean single pass");
    static_assert(ROWS == 0 || (!HASH && !MP && NIMG == 1), "general rows: Lloyd without hashing, one pass");
    // the gather's explicit vmcnt waits assume no other vector loads in the chain
    static_assert(!(GATH && ROWS == 2), "fp64 rows re-read x in the chain: register loads of the winner rows");
    static_assert(!FAST || (MET == 0 && ROWS != 2 && NIMG == 1 && !GATH), "fast distance: euclidean, fp32 rows");
    static_assert(PF == 0 || (FAST && !MP && ROWS == 0 && FH_WAVES == FH_FAST_WAVES), "row prefetch: the FAST single-pass form");
    static_assert(HG == 4 || (HASH && MET == 0 && PF != 0 && HG >= 1 && HG < 4), "fewer live hash groups: the prefetching FAST form");
    constexpr bool PFR = (PF & 1) != 0, PFL = (PF & 2) != 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Kpad = a.Kpad;
    const bool fastd = FAST || a.fast_dist != 0;
    const int KI = NIMG == 2 ? FH_KMAX : Kpad;           // centroid rows the LDS image holds
    int* lcount = reinterpret_cast<int*>(smem);          // [0] uncertified rows, [1] hash fix-up rows, [2] cosine declines
    _Float16* lch = reinterpret_cast<_Float16*>(smem + 16);
    float* lcn = reinterpret_cast<float*>(lch + KI * FU_RS);
    _Float16* lvh = reinterpret_cast<_Float16*>(lcn + KI);
    _Float16* lvl = lvh + 32 * FU_RS;
    float* lpn0 = reinterpret_cast<float*>(lvl + 32 * FU_RS);
    float* lv10 = lpn0 + 32;
    float* lt0 = lv10 + 32;
    int32_t* lr0 = reinterpret_cast<int32_t*>(lt0 + 32);

    // image img: centroid rows [img * KI, img * KI + rows) into LDS rows 0..
    auto load_image = [&](int img) {
        const int r0 = img * KI, nr = NIMG == 2 && img == 1 ? Kpad - FH_KMAX : KI;
        // FH_CU granules per thread in flight at once (a plain copy loop waited on every load)
        constexpr int FH_CU = 8;
        for (int e0 = 0; e0 < nr * 16; e0 += FH_THREADS * FH_CU) {
            float4 v[FH_CU];
#pragma unroll
            for (int u = 0; u < FH_CU; u++) {
                // past the end: granule 0 again (the same bytes rewritten), so neither
                // the loads nor the stores carry a branch and the loads issue together
                const int e = e0 + u * FH_THREADS + (int)threadIdx.x < nr * 16 ? e0 + u * FH_THREADS + (int)threadIdx.x : 0;
                v[u] = *reinterpret_cast<const float4*>(a.Ch + (size_t)(r0 + (e >> 4)) * FU_D + (e & 15) * 8);
            }
#pragma unroll
            for (int u = 0; u < FH_CU; u++) {
                const int e = e0 + u * FH_THREADS + (int)threadIdx.x < nr * 16 ? e0 + u * FH_THREADS + (int)threadIdx.x : 0;
                *reinterpret_cast<float4*>(lch + (e >> 4) * FU_RS + (e & 15) * 8) = v[u];
            }
        }
        for (int e = threadIdx.x; e < nr; e += FH_THREADS) lcn[e] = a.cnh[r0 + e];
    };
    load_image(0);
    if (threadIdx.x < 3) lcount[threadIdx.x] = 0;
    int32_t* ambig_seg = a.ambig + (int64_t)blockIdx.x * a.seg_rows;
    unsigned long long* hfix_seg = a.hfix + (int64_t)blockIdx.x * a.seg_rows;
    unsigned long long* cfix_seg = a.cfix ? a.cfix + (int64_t)blockIdx.x * a.seg_rows : nullptr;
    if (HASH) {
        hash_stage_images<FH_THREADS>(a.Vh, a.Vl, lvh, lvl);
        if (threadIdx.x < 32) {
            const int f = threadIdx.x;
            const bool on = f < a.LK;
            float P = 0.f, Q = 0.f;
            if (on) hash_window<MET == 0>(a.pnorm[f], a.v1[f], MET == 0 ? a.tv[f] : 0.f, a.w, P, Q);
            lpn0[f] = P;
            lv10[f] = Q;
            lt0[f] = on && MET == 0 ? a.tv[f] : 0.f;
            lr0[f] = on && MET == 0 ? a.rv[f] : 0;
        }
    }
    __syncthreads();

    // PF: the wave index as a scalar, so the tile index and "this wave has a next
    // tile" are uniform to the compiler: its two cases are then the arms of one
    // scalar branch, and no path exists that issues neither arm's loads (with
    // exec-masked arms the join assumed one, and waited the prefetch out).
    const int lane = threadIdx.x & 63;
    const int wave = PF != 0 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
    const int col = lane & 31, h = lane >> 5;
    const float cmaxf = a.cbound[3], crf = a.cbound[4], chf = a.cbound[5], cnf = a.cbound[6];
    const bool c_ok = __float_as_uint(a.cbound[2]) == 0u;
    const _Float16* my_h = lch + col * FU_RS + 8 * h;
    const int ntile32 = Kpad >> 5;
    const int64_t ntiles = (a.N + 31) >> 5;
    // point-independent part of the bound
    const double Ec = (0x1p-24 + FH_A) * (double)cnf + 0x1p-41 * (double)cmaxf * (double)cmaxf + 0x1p-18 * (double)cnf;

    const int64_t tstride = (int64_t)gridDim.x * FH_WAVES, tfirst = (int64_t)blockIdx.x * FH_WAVES;
    const int64_t nround = NIMG == 2 && ntiles > tfirst ? (ntiles - tfirst + tstride - 1) / tstride : 0;
    int64_t rd = 0;
    // profiling build: [0] row load + split + hash tile, [1] centroid tiles, [2] certificate + winner chain + stores
    // this lane's 64 values of row (tile, col) in the B-operand layout (rows past
    // the end read row N-1: their results are never stored)
    auto load_row = [&](int64_t tl, float (&dst)[64]) {
        const int64_t rr = tl * 32 + col, rc = rr < a.N ? rr : a.N - 1;
        if constexpr (ROWS != 0) load_row_gen<ROWS>(a, rc, h, dst);
        else load_row_b(a.X + rc * FU_D + 8 * h, dst);
    };
    // half hf (dims 64 hf .. + 63) of load_row: 8 loads of 16 B
    auto load_half = [&](int64_t tl, int hf, float* dst) {
        const int64_t rr = tl * 32 + col, rc = rr < a.N ? rr : a.N - 1;
        const float* xr = a.X + rc * FU_D + 64 * hf + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const float4 p0 = *reinterpret_cast<const float4*>(xr + 16 * s);
            const float4 p1 = *reinterpret_cast<const float4*>(xr + 16 * s + 4);
            dst[8 * s + 0] = p0.x; dst[8 * s + 1] = p0.y; dst[8 * s + 2] = p0.z; dst[8 * s + 3] = p0.w;
            dst[8 * s + 4] = p1.x; dst[8 * s + 5] = p1.y; dst[8 * s + 6] = p1.z; dst[8 * s + 7] = p1.w;
        }
    };
    // the lower halves of tile tl's rows into this wave's buffer: piece u holds
    // rows 4u..4u+3, lane L position L & 15 of row p = 4u + (L >> 4), that is
    // chunk (L & 15) ^ (p & 15) of the row (clamped to N - 1 as load_row's)
    uint32_t pfbase = 0;
    if constexpr (PFL)
        pfbase = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)((uint32_t)(uintptr_t)(smem + fh_rowpf_off(Kpad, HASH)) + (uint32_t)wave * FH_ROWPF_WAVE));
    // The tile's first row is a scalar base (tl is the same in every lane), the
    // lane's part a 32-bit offset: no 64-bit address registers per piece.
    auto pf_dma = [&](int64_t tl) {
        const int64_t tls = ((int64_t)__builtin_amdgcn_readfirstlane((int)(tl >> 32)) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane((int)tl);
        const int64_t left = a.N - 1 - tls * 32;             // >= 0: tl < ntiles
        const int pmax = left < 31 ? (int)left : 31;
        const float* xt = a.X + tls * 32 * FU_D;
        if (pmax == 31) {
            // every row of the tile exists (a scalar test). With q = L >> 4 (< 4), c =
            // L & 15: p & 15 = 4 (u & 3) | q, so piece u's lane offset is
            // u * 2048 + (w0 ^ 64 (u & 3)), w0 = 512 q + 16 (c ^ q) the same for every
            // tile (the xor touches bits 6..7, 512 q bits 9..10): one VALU instruction
            // per piece, the piece's rows on the scalar base.
            const uint32_t w0 = (uint32_t)((lane >> 4) * (FU_D * 4) + 16 * ((lane & 15) ^ (lane >> 4)));
#pragma unroll
            for (int u = 0; u < 8; u++) glds16s(xt + u * 4 * FU_D, w0 ^ (uint32_t)(64 * (u & 3)), pfbase, u * 1024);
        } else {
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int p = 4 * u + (lane >> 4), pc = p < pmax ? p : pmax;
                glds16s(xt, (uint32_t)(pc * (FU_D * 4) + 16 * ((lane & 15) ^ (p & 15))), pfbase, u * 1024);
            }
        }
    };
    // The next tile's fetch, issued between the hash phase and the centroid tiles
    // (both halves: the centroid loop leaves 32 registers free beside xf and bh).
    // WAR: the DMA refills the buffer only once this tile's reads of it have
    // returned (lgkmcnt(0), as ring_advance). Over-waiting: the issue sits behind
    // the last wait on the row registers -- a compiler wait for an older load
    // would not count the DMA and so wait it out too.
    // PFR: the upper halves of a wave's tiles live in two register sets that
    // trade places from tile to tile (the loop below runs over tile pairs): the
    // tile at hand computes from one while the next tile's loads land in the
    // other, so no copy takes them over. The wave's last tile fetches nothing,
    // and nothing reads the other set after it.
    float xua[32], xub[32];
    auto pf_next = [&](int64_t tl, float (&xnx)[32]) {
        if constexpr (PF != 0) {
            if (tl + tstride < ntiles) {
                if constexpr (PFL) {
                    __builtin_amdgcn_s_waitcnt(0xC07F);                    // lgkmcnt(0)
                    asm volatile("" ::: "memory");
                    pf_dma(tl + tstride);
                }
                if constexpr (PFR) load_half(tl + tstride, 1, xnx);
            }
        }
    };
    // Prologue: the wave's first tile both ways, waited out here (vmcnt(0), once
    // per wave), so that at every loop top the fetch is either complete or has
    // the winner distance's 16 centroid loads behind it (the top's wait below).
    if constexpr (PF != 0) {
        if (tfirst + wave < ntiles) {
            if constexpr (PFL) pf_dma(tfirst + wave);
            if constexpr (PFR) load_half(tfirst + wave, 1, xua);
            if constexpr (PFL) {
                __builtin_amdgcn_s_waitcnt(0x0F70);                        // vmcnt(0)
                asm volatile("" ::: "memory");
            }
        }
    }
    PT_DECL
    // One tile. xup: the tile's upper halves (PFR), xnx: where the next tile's go.
    auto tile_body = [&](const int64_t tile, float (&xup)[32], float (&xnx)[32]) __attribute__((always_inline)) {
        const int64_t row = tile * 32 + col;
        const bool valid = row < a.N;
        // dims 0..63 of the lane's share in xf[0..31]; dims 64..127 in xf[32..63],
        // or with PFR in xup (xf's upper half is then never touched)
        float xf[64];
        float* const xhi = PFR ? xup : xf + 32;
        auto x8 = [&](int s) -> const float* { return s < 4 ? xf + 8 * s : xhi + 8 * (s - 4); };
        if constexpr (PF == 0) {
            load_row(tile, xf);
        } else {
            if constexpr (PFL) {
                if constexpr (!PFR) {
                    load_half(tile, 1, xf + 32);
                    asm volatile("" ::: "memory");            // the 8 loads stay above the wait that counts them
                }
                // RAW: only this wave's covering vmcnt wait orders the reads behind the
                // tile's DMA. vmcnt(n) waits for all but the n youngest vector-memory
                // operations, so n may only be a lower bound, on every path from the
                // DMA's issue to here, of those issued after it:
                //  - from the prologue: none, and the prologue has waited the DMA out;
                //  - from pf_next a tile ago: the 16 centroid-row loads of the winner
                //    distance (fastd is compiled in: unconditional, 16 instructions of
                //    16 B); rn32's load, the stores and the list appends are conditional
                //    or may be moved, and are not counted;
                //  - without the register half, the 8 loads just issued above instead.
                // The pair loop has two copies of this top. Each is reached from exactly
                // one pf_next: the second tile's from the first tile's (straight down the
                // pair), the first tile's from the second tile's (round the loop), or from
                // the prologue on the wave's first tile; a single last tile leaves through
                // the first copy's "no next tile" arm, having issued nothing. Every such
                // path runs one whole tile body after the DMA, with that body's 16
                // centroid-row loads, so the count is 16 in both copies. The register
                // half (8 loads, issued after the DMA and before those 16) is older than
                // the 16 as well: the same wait covers the set this tile reads.
                // vmcnt(16) therefore leaves this tile's own stores in flight and waits
                // for nothing younger than the centroid rows, which the distance has
                // consumed: the wait is a guard, not a stall.
                __builtin_amdgcn_s_waitcnt(PFR ? 0x4F70 : 0x0F78);                 // vmcnt(16) : vmcnt(8)
                asm volatile("" ::: "memory");
                const char* pb = smem + fh_rowpf_off(Kpad, HASH) + wave * FH_ROWPF_WAVE + col * 256;
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    const float4 v = *reinterpret_cast<const float4*>(pb + 16 * ((4 * (c >> 1) + 2 * h + (c & 1)) ^ (col & 15)));
                    xf[4 * c] = v.x; xf[4 * c + 1] = v.y; xf[4 * c + 2] = v.z; xf[4 * c + 3] = v.w;
                }
            } else {
                load_half(tile, 0, xf);
            }
        }
        half8 bh[8];
        float2v n2a = {0.f, 0.f}, n2b = {0.f, 0.f}, r2 = {0.f, 0.f};
        double xn2, nx, nxr, nxh;
        bool x_ok;
        auto finish_norms = [&]() {
            float xn2f = (n2a.x + n2a.y) + (n2b.x + n2b.y);
            float xr2f = r2.x + r2.y;
            xn2f += __shfl_xor(xn2f, 32);
            xr2f += __shfl_xor(xr2f, 32);
            // f32 sums of squares inflated by 2^-16 (> d 2^-24): upper bounds
            xn2 = (double)xn2f * (1.0 + 0x1p-16);
            nx = sqrt(xn2);
            nxr = sqrt((double)xr2f * (1.0 + 0x1p-16)) + 0x1p-100;
            if (ROWS == 2) nxr += 0x1p-24 * nx * (1.0 + 0x1p-20);   // |x - f32(x)| (fp64 rows)
            nxh = nx + nxr;                                     // |xh| <= |x| + |xr|
            x_ok = xn2f <= FU_RANGE * FU_RANGE;
        };
        const bool hash_here = HASH;          // <HASH, MP>: the first pass only
        if (!hash_here) {
#pragma unroll
            for (int s = 0; s < 8; s++) {
                half8 unused;
                split_norm_step<false>(x8(s), bh[s], unused, n2a, n2b, r2);
            }
            pf_next(tile, xnx);
            finish_norms();
        }

        if (hash_here) {
            uint32_t fmask = 0;
            float acc_hi[16];
            {
                const _Float16* vh_row = lvh + col * FU_RS + 8 * h;
                const _Float16* vl_row = lvl + col * FU_RS + 8 * h;
                floatx16 tot;
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    half8 bl;
                    split_norm_step<true>(x8(s), bh[s], bl, n2a, n2b, r2);
                    const floatx16 acc = hash_tile_step(s, vh_row, vl_row, bh[s], bl);
                    if (s == 0) {
                        tot = acc;
                    } else {
                        // the live groups only (HG): the others hold padding rows
#pragma unroll
                        for (int r = 0; r < 4 * HG; r += 2) {
                            const float2v t2 = {tot[r], tot[r + 1]}, a2 = {acc[r], acc[r + 1]};
                            const float2v u2 = t2 + a2;
                            tot[r] = u2.x;
                            tot[r + 1] = u2.y;
                        }
                    }
                }
                // HG < 4: registers 4 HG.. keep step 0's partial values; no group g >= HG reads them
#pragma unroll
                for (int r = 0; r < 16; r++) acc_hi[r] = tot[r];
            }
            finish_norms();
            // hash_tile.h's certificates; hc, an opaque zero, keeps the per-function
            // constants as LDS reads inside the loop instead of hoisted VGPRs.
            const float iw = MET == 1 ? 1.f : 1.0f / a.w;
            const float nxf = (float)nx * (1.f + 0x1p-20f);
            int hc = 0;
            asm volatile("" : "+v"(hc));
            // cosine reads P and Q per function (declared here, outside the loop: inside it
            // the cosine kernels' register allocation changes, and they are not re-measured)
            const float* lP = lpn0 + hc;
            const float* lQ = lv10 + hc;
            // euclidean: P, Q, t, r are four arrays of 32 in a row (lpn0, lv10, lt0,
            // lr0), so the constants of table 2g + h's four functions are four 16-B
            // reads off one base, at the immediate offsets 128 j + 32 g bytes
            const float* hb = lpn0 + hc + 4 * h;
            if (!x_ok && valid) fmask = (a.LK >= 32 ? 0xFFFFFFFFu : (1u << a.LK) - 1u);
#pragma unroll
            for (int g = 0; g < HG; g++) {
                const int l = 2 * g + h;
                if (l >= a.L || !valid) continue;
                const int64_t o = row * a.L + l;
                if constexpr (MET == 1) {
                    // CosineHGen: ip >= 0, certified when |acc~| exceeds the window;
                    // CosineGGen: g = bits MSB first
                    int gv = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int f = 4 * l + q;
                        int bit;
                        if (!certify_sign_f32(acc_hi[4 * g + q], nxf, lP[f], lQ[f], bit)) fmask |= 1u << f;
                        gv = (gv << 1) | bit;
                    }
                    if (a.phi) a.phi[o] = gv;
                    if (a.bucket) a.bucket[o] = gv;
                    continue;
                }
                const float4 P4 = *reinterpret_cast<const float4*>(hb + 8 * g);
                const float4 Q4 = *reinterpret_cast<const float4*>(hb + 32 + 8 * g);
                const float4 t4 = *reinterpret_cast<const float4*>(hb + 64 + 8 * g);
                const int4 r4 = *reinterpret_cast<const int4*>(hb + 96 + 8 * g);
                int32_t hv[4];
                fmask |= certify_floor4_f32(acc_hi + 4 * g, t4, iw, nxf, P4, Q4, hv) << (4 * l);
                if (a.tuples) *reinterpret_cast<int4*>(a.tuples + o * 4) = make_int4(hv[0], hv[1], hv[2], hv[3]);
                const int32_t rv4[4] = {r4.x, r4.y, r4.z, r4.w};
                const uint32_t ph = phi_final(phi_sum4_small(hv, rv4));
                if (a.phi) a.phi[o] = (int32_t)ph;
                if (a.bucket) a.bucket[o] = bucket_fast(ph, a.bdiv);
            }
            fmask |= __shfl_xor(fmask, 32);
            const unsigned long long fb = __ballot(fmask != 0u && h == 1);
            if (fb) {
                const int leader = __builtin_ctzll(fb);
                int base = 0;
                if (lane == leader) base = atomicAdd(lcount + 1, __popcll(fb));
                base = __shfl(base, leader);
                if (fmask != 0u && h == 1)
                    hfix_seg[base + __popcll(fb & ((1ull << lane) - 1ull))] = ((unsigned long long)row << 32) | fmask;
            }
        }

        if (HASH) pf_next(tile, xnx);
        PT_MARK(0)
        // the certificate's bound E depends on the row only: formed before the
        // centroid tiles (its fp64 ops overlap the MFMAs). cosine: + 2^-43 |x| for the normalisation and the reference's own q
        // (fused_persistent_kernel's cosine bound)
        const double E = (nxh * (double)crf + nxr * (double)cmaxf + FH_A * nxh * (double)chf + 0x1p-41 * xn2 +
                          0x1p-18 * nx * (double)cmaxf + (MET == 1 ? 0x1p-43 * nx : 0.0) + Ec) * (1.0 + 0x1p-20) +
                         1e-30;
        // ---- centroid tiles: 8 MFMAs each, accumulator initialised with -|c|^2/2
        float m1 = -__builtin_inff(), m2 = -__builtin_inff();
        int t1 = 0;
        if (MP && !HASH && !a.pass_first) {
            const float4 st = a.part[tile * 64 + lane];
            m1 = st.x; m2 = st.y; t1 = __float_as_int(st.z);
        }
        const int tg0 = MP ? a.t0 : 0;
        __builtin_amdgcn_s_setprio(MFMA_PRIO);
        const int ntile_run = ntile32;
        auto run_tiles = [&](int ntl, int tgo) {
#pragma unroll 1
            for (int t = 0; t < ntl; t++) {
                const float m1_prev = m1;
                floatx16 acc;
                const float* cn_t = lcn + t * 32 + 4 * h;     // D rows 8g + 4h + q of registers 4g + q
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const float4 cn = *reinterpret_cast<const float4*>(cn_t + 8 * g);
                    acc[4 * g] = cn.x; acc[4 * g + 1] = cn.y; acc[4 * g + 2] = cn.z; acc[4 * g + 3] = cn.w;
                }
                const _Float16* arow = my_h + t * 32 * FU_RS;
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const half8 ah = *reinterpret_cast<const half8*>(arow + 16 * s);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[s], acc, 0, 0, 0);
                }
                float sv[16];
#pragma unroll
                for (int r = 0; r < 16; r++) sv[r] = acc[r];
                tile_epilogue(sv, m1, m2);
                t1 = m1 != m1_prev ? t + tgo : t1;
            }
        };
        if (NIMG == 1) {
            run_tiles(ntile_run, tg0);
        } else {
            // the image in LDS at this round's start, then the other one
            const int i0 = (int)(rd & 1);
            const int nA = FH_KMAX / 32, nB = (Kpad - FH_KMAX) / 32;
            run_tiles(i0 == 0 ? nA : nB, i0 * nA);
            __syncthreads();
            load_image(1 - i0);
            __syncthreads();
            run_tiles(i0 == 0 ? nB : nA, (1 - i0) * nA);
        }
        __builtin_amdgcn_s_setprio(0);
        PT_MARK(1)
        // <HASH, MP> launches only the first of several passes (never the last)
        if (MP && (HASH || !a.pass_last)) {
            a.part[tile * 64 + lane] = make_float4(m1, m2, __int_as_float(t1), 0.f);
            return;
        }
        const uint32_t l1 = __float_as_uint(m1) & 0xFu;
        const int i1 = t1 * 32 + 8 * (int)(l1 >> 2) + 4 * h + (int)(l1 & 3u);
        const float om1 = __shfl_xor(m1, 32), om2 = __shfl_xor(m2, 32);
        const int oi1 = __shfl_xor(i1, 32);
        const float M2 = fmaxf(fmaxf(m2, om2), fminf(m1, om1));
        const int I1 = (om1 > m1 || (om1 == m1 && oi1 < i1)) ? oi1 : i1;
        const float M1 = fmaxf(m1, om1);
        // the winner's fp64 row: the first loads go out before the certificate
        // and the list append
        const double* crow = a.C64 + (size_t)I1 * FU_D + 8 * h;
        // GATH: piece u of a step holds points 8u..8u+7, lane L the 16-B chunk
        // (L & 7) ^ swz(p) of point p = 8u + (L >> 3) (swz(p) = (p >> 1) & 7: the
        // lanes of each ds_read_b128 group hit 16 distinct 4-bank groups).
        // g32 (every centroid value is an f32, e.g. dataset rows: the prep's
        // cbound[7] == 0): the f32 image C32 instead, exact as doubles -- half the
        // bytes and two pieces per step: piece u holds points 16u..16u+15, lane L
        // the 16-B chunk (L & 3) ^ swz32(p) of point p = 16u + (L >> 2), swz32(p) =
        // (p >> 2) & 3 (the 16 lanes of a ds_read_b128 group on distinct banks).
        const char* gsrc[4];
        uint32_t gbase = 0;
        const bool g32 = GATH && a.C32 != nullptr && (__float_as_uint(a.cbound[7]) & 1u) == 0u;
        const int gstep = g32 ? 64 : 128;                // bytes of one 16-dim step of a row
        if (GATH && !fastd) {
            gbase = (uint32_t)__builtin_amdgcn_readfirstlane(
                (int)((uint32_t)(uintptr_t)(smem + fh_gath_off(Kpad, HASH)) + (uint32_t)wave * FH_GATH_WAVE));
            if (g32) {
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int p = 16 * u + (lane >> 2);
                    const int Ip = __shfl(I1, p);
                    gsrc[u] = reinterpret_cast<const char*>(a.C32 + (size_t)Ip * FU_D + 4 * ((lane & 3) ^ ((p >> 2) & 3)));
                }
                gsrc[2] = gsrc[3] = gsrc[0];
#pragma unroll
                for (int s0 = 0; s0 < 2; s0++)
#pragma unroll
                    for (int u = 0; u < 2; u++) glds16(gsrc[u] + gstep * s0, gbase + s0 * FH_GATH_STEP + u * 1024);
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int p = 8 * u + (lane >> 3);
                    const int Ip = __shfl(I1, p);
                    gsrc[u] = reinterpret_cast<const char*>(a.C64 + (size_t)Ip * FU_D + 2 * ((lane & 7) ^ ((p >> 1) & 7)));
                }
#pragma unroll
                for (int s0 = 0; s0 < 2; s0++)
#pragma unroll
                    for (int u = 0; u < 4; u++) glds16(gsrc[u] + gstep * s0, gbase + s0 * FH_GATH_STEP + u * 1024);
            }
        }
        // GATH: a step's values come from the ring one step early (the LDS read
        // overlaps the previous step's chain), the ring slot is refilled two
        // steps ahead as soon as it is read
        double2 gnext[4];
        float4 gnext32[2];                    // g32: raw f32 chunks, widened when used
        auto gread = [&](int st) {
            const char* ring = smem + fh_gath_off(Kpad, HASH) + wave * FH_GATH_WAVE + (st & 1) * FH_GATH_STEP;
            if (g32) {
#pragma unroll
                for (int j = 0; j < 2; j++)
                    gnext32[j] = *reinterpret_cast<const float4*>(ring + (col >> 4) * 1024 + (col & 15) * 64 +
                                                                  16 * ((2 * h + j) ^ ((col >> 2) & 3)));
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    gnext[j] = *reinterpret_cast<const double2*>(ring + col * 128 + 16 * ((4 * h + j) ^ ((col >> 1) & 7)));
            }
        };
        // vmcnt(n): all but the wave's n youngest vector-memory operations done
        // (one step's pieces: 2 for g32, else 4)
        auto wait_step = [&]() {
            if (g32) __builtin_amdgcn_s_waitcnt(0x0F72);                   // vmcnt(2)
            else __builtin_amdgcn_s_waitcnt(0x0F74);                       // vmcnt(4)
        };
        // ring step s consumed: slot s & 1 refilled with step s + 2, step s + 1 read
        auto ring_advance = [&](int s) {
            if (s + 2 < 8) {
                __builtin_amdgcn_s_waitcnt(0xC07F);                        // lgkmcnt(0): slot s & 1 is read
                asm volatile("" ::: "memory");
                if (g32) {
#pragma unroll
                    for (int u = 0; u < 2; u++) glds16(gsrc[u] + gstep * (s + 2), gbase + (s & 1) * FH_GATH_STEP + u * 1024);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; u++) glds16(gsrc[u] + gstep * (s + 2), gbase + (s & 1) * FH_GATH_STEP + u * 1024);
                }
            }
            if (s + 1 < 8) {
                if (s + 2 < 8) wait_step();                                // step s + 1 landed
                else __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0)
                asm volatile("" ::: "memory");
                gread(s + 1);
            }
        };
        // fp64 rows: the chain's x values re-read (mostly L2) four 16-dim steps
        // ahead (one step ahead left the chain waiting ~8 round trips per tile)
        constexpr int XD = 4;
        double2 xring[XD][4];
        const int64_t rowc = row < a.N ? row : a.N - 1;
        if constexpr (ROWS == 2 && MET == 0) {
#pragma unroll
            for (int st = 0; st < XD; st++) load_x64_step(a, rowc, st, h, xring[st]);
        }
        // the winner's fp64 row, one 16-dim step ahead of the chain (deeper
        // prefetch measured slower: DESIGN.md)
        double2 cbuf[4];
        if (MET == 0 && !GATH && !fastd) {
#pragma unroll
            for (int j = 0; j < 4; j++) cbuf[j] = *reinterpret_cast<const double2*>(crow + 2 * j);
        }
        const bool cert = x_ok && c_ok && ((double)M2 < (double)M1 - 2.0 * E);

        // euclidean fast distance (fastd): the winner's distance from f32(c)
        // in f32 with every lane busy, certified to 2^-20 relative (DESIGN.md §5:
        // 8 accumulators per lane, <= 12 roundings per sum, plus the f32(c)
        // residual |c - f32(c)| of the centroid); a row whose bound fails is
        // refined like an uncertified argmin (the exact chain of the refinement)
        bool dok = true;
        double fdist = 0.0;
        if constexpr (MET == 0) {
            if (fastd) {
                const float* c32 = a.C32 + (size_t)I1 * FU_D + 8 * h;
                float2v q[4] = {};
                // PF: the 16 loads issued together, as the form without the prefetch has
                // them (with the next tile's register set live the scheduler otherwise
                // takes them two at a time, eight L2 round trips in a row)
                float4 cc[16];
                if constexpr (PF != 0) {
#pragma unroll
                    for (int s = 0; s < 8; s++) {
                        cc[2 * s] = *reinterpret_cast<const float4*>(c32 + 16 * s);
                        cc[2 * s + 1] = *reinterpret_cast<const float4*>(c32 + 16 * s + 4);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    float4 c0, c1;
                    if constexpr (PF != 0) {
                        c0 = cc[2 * s]; c1 = cc[2 * s + 1];
                    } else {
                        c0 = *reinterpret_cast<const float4*>(c32 + 16 * s);
                        c1 = *reinterpret_cast<const float4*>(c32 + 16 * s + 4);
                    }
                    const float2v cv[4] = {{c0.x, c0.y}, {c0.z, c0.w}, {c1.x, c1.y}, {c1.z, c1.w}};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float2v xv = {x8(s)[2 * j], x8(s)[2 * j + 1]};
                        const float2v dv = xv - cv[j];
                        q[j] = __builtin_elementwise_fma(dv, dv, q[j]);
                    }
                }
                float t = ((q[0].x + q[0].y) + (q[1].x + q[1].y)) + ((q[2].x + q[2].y) + (q[3].x + q[3].y));
                t = t + swap_halves_f(t, h);
                const double S = (double)t, R = (double)a.rn32[I1];
                const double B = 14.2 * 0x1p-24 * S + 2.02 * R * sqrt(S) + 2.02 * R * R + 0x1p-100;
                dok = B <= 0x1p-19 * S;                   // false for inf / nan
                fdist = sqrt(S);
            }
        }
        const bool amb = valid && !(cert && dok);
        const unsigned long long amask = __ballot(amb && h == 1);
        if (amb && h == 1) {
            int base = 0;
            const int leader = __builtin_ctzll(amask);
            if (lane == leader) base = atomicAdd(lcount, __popcll(amask));
            base = __shfl(base, leader);
            ambig_seg[base + __popcll(amask & ((1ull << lane) - 1ull))] = (int32_t)row;
        }
        if constexpr (MET == 1) {
            // cosine winner from the row in registers, both lane halves busy;
            // declined certificates -> the fix-up list
            bool fix = false;
            if (valid && cert) {                          // the same on both halves of a point
                double v = 0.0;
                int st;
                // fp32 rows (ROWS = 0 / 1): the values in registers are exact (zero
                // past d, as the padded centroid copy); fp64 rows re-read
                if constexpr (ROWS == 2) st = cosine_winner_halves_x64(a, row, a.C64 + (size_t)I1 * FU_D + 8 * h, a.nbv[I1], h, v);
                else st = cosine_winner_halves(xf, a.C64 + (size_t)I1 * FU_D + 8 * h, a.nbv[I1], h, v);
                if (h == 1) {
                    a.assign[row] = I1;
                    if (st == 0) a.dist[row] = v;
                    else fix = true;
                }
            }
            const unsigned long long fb = __ballot(fix);
            if (fb) {
                const int leader = __builtin_ctzll(fb);
                int base = 0;
                if (lane == leader) base = atomicAdd(lcount + 2, __popcll(fb));
                base = __shfl(base, leader);
                if (fix) cfix_seg[base + __popcll(fb & ((1ull << lane) - 1ull))] = (unsigned long long)row;
            }
        } else if (fastd) {
            if (h == 1 && valid && cert && dok) {
                a.assign[row] = I1;
                a.dist[row] = fdist;
            }
        } else {
            // winner distance in reference order from the row kept in registers:
            // the lane halves take turns on the chain, 8 dims each
            __builtin_amdgcn_s_setprio(CHAIN_PRIO);
            double acc = 0.0;
            PwAcc pw;
            // fp64 rows: glibc's pow in the chain itself when the launch gave the
            // LDS for it (gp_sq_wave; every difference of general doubles has
            // more than 26 bits, so the PwAcc test would list every row)
            double* pwl = nullptr;
            if constexpr (ROWS == 2) {
                if (a.pw_lds) pwl = reinterpret_cast<double*>(smem + a.pw_lds) + wave * 512;
            }
            if constexpr (GATH) {
                wait_step();                                               // step 0 landed
                asm volatile("" ::: "memory");
                gread(0);
            }
#pragma unroll
            for (int s = 0; s < 8; s++) {
                double sq[8];
                double2 cur[4];
                if constexpr (GATH) {
                    if (g32) {
#pragma unroll
                        for (int j = 0; j < 2; j++) {
                            cur[2 * j] = make_double2((double)gnext32[j].x, (double)gnext32[j].y);
                            cur[2 * j + 1] = make_double2((double)gnext32[j].z, (double)gnext32[j].w);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; j++) cur[j] = gnext[j];
                    }
                    ring_advance(s);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) cur[j] = cbuf[j];
                    if (s + 1 < 8) {
#pragma unroll
                        for (int j = 0; j < 4; j++) cbuf[j] = *reinterpret_cast<const double2*>(crow + 16 * (s + 1) + 2 * j);
                    }
                }
                double2 xcur[4];
                if constexpr (ROWS == 2) {
#pragma unroll
                    for (int j = 0; j < 4; j++) xcur[j] = xring[s % XD][j];
                    if (s + XD < 8) load_x64_step(a, rowc, s + XD, h, xring[s % XD]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) xcur[j] = make_double2((double)x8(s)[2 * j], (double)x8(s)[2 * j + 1]);
                }
                double dv[8];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double2 cc = cur[j];
                    dv[2 * j] = __dsub_rn(xcur[j].x, cc.x);
                    dv[2 * j + 1] = __dsub_rn(xcur[j].y, cc.y);
                }
                if (ROWS == 2 && pwl) {
                    gp_sq_wave<8>(dv, sq, pwl);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        sq[j] = __dmul_rn(dv[j], dv[j]);
                        // the reference squares with glibc pow: x*x is its value when
                        // the square is exact; otherwise the row's distance is redone
                        // by the fix-up (gpow2.h PwAcc: differences of <= 26 bits, and
                        // for fp64 rows no tiny ones)
                        pw.add<ROWS == 2>(dv[j]);
                    }
                }
                if (h == 0) {
#pragma unroll
                    for (int j = 0; j < 8; j++) acc = __dadd_rn(acc, sq[j]);
                }
                acc = take_from_lower(acc);
                if (h == 1) {
#pragma unroll
                    for (int j = 0; j < 8; j++) acc = __dadd_rn(acc, sq[j]);
                }
                acc = take_from_upper(acc);
            }
            // fp32 rows: a difference 0 < |x - c| < 2^-460 needs such a centroid
            // value (x has >= 2^-149 magnitude or is zero), flagged by the prep
            const bool pw_hard = pwl == nullptr && (pw.hard() || (ROWS != 2 && (__float_as_uint(a.cbound[7]) & 2u) != 0u));
            // the shuffle outside the ||: evaluated only where pw_hard is false, it
            // would read the other half's lane while that lane is masked off
            const int pw_other = __shfl_xor((int)pw_hard, 32);
            const bool hard = pw_hard || pw_other != 0;
            if (h == 1 && valid && cert) {
                a.assign[row] = I1;
                if (!hard) a.dist[row] = sqrt(acc);
            }
            // the pow fix-up list (cfix, counts in slot 2): certified winners
            // whose chain met an inexact square
            const unsigned long long pb = __ballot(h == 1 && valid && cert && hard);
            if (pb) {
                const int leader = __builtin_ctzll(pb);
                int base = 0;
                if (lane == leader) base = atomicAdd(lcount + 2, __popcll(pb));
                base = __shfl(base, leader);
                if (h == 1 && valid && cert && hard) cfix_seg[base + __popcll(pb & ((1ull << lane) - 1ull))] = (unsigned long long)row;
            }
            __builtin_amdgcn_s_setprio(0);
        }
        PT_MARK(2)
    };
    if constexpr (PFR) {
        // Tile pairs: the first tile reads xua while the second's loads land in
        // xub, the second reads xub while the next pair's first lands in xua. The
        // wave's tile count may be odd: its last tile runs the first copy alone.
        // "Has a next tile" is a scalar test (the wave index is one), here and in
        // pf_next alike.
        for (int64_t tile = tfirst + wave; tile < ntiles; tile += 2 * tstride) {
            tile_body(tile, xua, xub);
            if (tile + tstride >= ntiles) break;
            tile_body(tile + tstride, xub, xua);
        }
    } else {
        for (int64_t tile = tfirst + wave; NIMG == 2 ? rd < nround : tile < ntiles; tile += tstride, rd++)
            tile_body(tile, xua, xub);
    }
    PT_FLUSH
    __syncthreads();
    // thread t writes slot t: SEG_ROWS (uncertified rows), SEG_FIX (hash fix-ups)
    if (threadIdx.x < 2 && (!MP || (threadIdx.x == 0 ? (!HASH && a.pass_last != 0) : (HASH && a.pass_first)))) {
        const int c = lcount[threadIdx.x];
        a.seg_counts[SEG_SLOTS * blockIdx.x + threadIdx.x] = c;
        if (c) atomicAdd(threadIdx.x == 0 ? a.ambig_count : a.hfix_count, (unsigned long long)c);
    }
    // slot 2: cosine declines / euclidean pow fix-ups (exact distances)
    if ((MET == 1 || !fastd) && threadIdx.x == 2 && (!MP || (!HASH && a.pass_last))) {
        const int c = lcount[2];
        a.cfix_counts[SEG_SLOTS * blockIdx.x + SEG_FIX] = c;
        if (c) atomicAdd(a.cfix_count, (unsigned long long)c);
    }
}

template <bool HASH, bool MP, int MET, int NIMG, bool GATH, int ROWS, bool FAST, int PF, int HG>
static void hi_launch(hipStream_t s, unsigned nblk, size_t lds, const FusedArgs& a) {
    hipLaunchKernelGGL((fused_hi_kernel<HASH, MP, MET, NIMG, GATH, ROWS, FAST, PF, HG>), dim3(nblk),
                       dim3(64 * fh_waves<HASH, MP, MET, FAST>()), lds, s, a);
}

int launch_fused_hi_pass(hipStream_t s, unsigned nblk, const HiForm& f, FusedArgs a) {
    // LDS: the image (+ the hash rows), then the gather ring or the fp64 chain's pow buffers
    size_t lds = (size_t)fh_lds_bytes(f.two_image ? FH_KMAX : a.Kpad, f.hash);
    a.pw_lds = 0;
    if (f.gath) {
        if (a.Kpad > FH_GATH_KMAX) {
            set_error("launch_fused_hi_pass: the gather ring needs K <= 256");
            return -1;
        }
        lds = (size_t)fh_gath_off(a.Kpad, f.hash) + 8 * FH_GATH_WAVE;
    } else if (f.rows == 2 && f.metric == 0) {
        // the chain's pow buffers after the image when they fit (Kpad <= 448)
        constexpr int PW_BYTES = fh_waves<false, false, 0>() * 512 * 8;
        const size_t off = (lds + 255) & ~(size_t)255;
        if (off + PW_BYTES <= 160 * 1024) {
            a.pw_lds = (int)off;
            lds = off + PW_BYTES;
        }
    }
    const int pf = f.rowpf ? FH_ROWPF : 0;
    if (pf != 0 && !(f.fast && !f.mp && f.rows == 0 && !f.gath && a.Kpad <= FH_ROWPF_KMAX)) {
        set_error("launch_fused_hi_pass: the row prefetch needs the fast single-pass form at K <= 256");
        return -1;
    }
    // the waves' row buffers after the image
    if (pf & 2) lds = (size_t)fh_rowpf_off(a.Kpad, f.hash) + FH_FAST_WAVES * FH_ROWPF_WAVE;
    const int nimg = f.two_image ? 2 : 1;
    // live hash groups: 3 for L = 5 or 6 on the prefetching FAST form (the headline shape), else all 4
    const int hg = f.hash && pf != 0 && (a.L == 5 || a.L == 6) ? 3 : 4;
    // every instantiation the library builds, one line each
#define HI_CASE_HG(H, MP, MET, NIMG, GATH, ROWS, FAST, PF, HG)                                              \
    if (f.hash == (bool)H && f.mp == (bool)MP && f.metric == MET && nimg == NIMG && f.gath == (bool)GATH && \
        f.rows == ROWS && f.fast == (bool)FAST && pf == PF && hg == HG) {                                   \
        hi_launch<H, MP, MET, NIMG, GATH, ROWS, FAST, PF, HG>(s, nblk, lds, a);                             \
        return 0;                                                                                           \
    }
#define HI_CASE_PF(H, MP, MET, NIMG, GATH, ROWS, FAST, PF) HI_CASE_HG(H, MP, MET, NIMG, GATH, ROWS, FAST, PF, 4)
#define HI_CASE(H, MP, MET, NIMG, GATH, ROWS, FAST) HI_CASE_PF(H, MP, MET, NIMG, GATH, ROWS, FAST, 0)
    //      hash mp met nimg gath rows fast (rows fetched a tile ahead) (live hash groups)
#if LSHKM_ROWPF != 0
    HI_CASE_HG(1, 0, 0, 1, 0, 0, 1, FH_ROWPF, 3)   // L = 5, 6: tables 6 and 7 are padding
#endif
    HI_CASE_PF(1, 0, 0, 1, 0, 0, 1, FH_ROWPF)   // euclidean, fp32 d = 128, one pass: the certified f32 distance
    HI_CASE_PF(0, 0, 0, 1, 0, 0, 1, FH_ROWPF)   // with its rows fetched one tile ahead,
    HI_CASE(1, 0, 0, 1, 0, 0, 1)      // or at the tile's top (the test build's LSHKM_ROW_PREFETCH=0),
    HI_CASE(0, 0, 0, 1, 0, 0, 1)
    HI_CASE(1, 0, 0, 1, 1, 0, 0)      // the exact chain through the gather ring,
    HI_CASE(0, 0, 0, 1, 1, 0, 0)
    HI_CASE(1, 0, 0, 1, 0, 0, 0)      // or by register loads (K > 256; tests)
    HI_CASE(0, 0, 0, 1, 0, 0, 0)
    HI_CASE(1, 1, 0, 1, 0, 0, 0)      // K > 512: the first pass hashes,
    HI_CASE(0, 1, 0, 1, 0, 0, 1)      // the last one may compile the f32 distance in
    HI_CASE(0, 1, 0, 1, 0, 0, 0)
    HI_CASE(1, 0, 0, 2, 0, 0, 0)      // two-image form (tests)
    HI_CASE(0, 0, 0, 2, 0, 0, 0)
    HI_CASE(1, 0, 1, 1, 0, 0, 0)      // cosine
    HI_CASE(0, 0, 1, 1, 0, 0, 0)
    HI_CASE(1, 1, 1, 1, 0, 0, 0)
    HI_CASE(0, 1, 1, 1, 0, 0, 0)
    HI_CASE(0, 0, 0, 1, 0, 1, 1)      // general rows: fp32 d <= 128
    HI_CASE(0, 0, 0, 1, 1, 1, 0)
    HI_CASE(0, 0, 0, 1, 0, 1, 0)
    HI_CASE(0, 0, 1, 1, 0, 1, 0)
    HI_CASE(0, 0, 0, 1, 0, 2, 0)      // general rows: fp64 d <= 128
    HI_CASE(0, 0, 1, 1, 0, 2, 0)
#undef HI_CASE
#undef HI_CASE_HG
#undef HI_CASE_PF
    set_error("launch_fused_hi_pass: no kernel was built for this form");
    return -1;
}

}  // namespace lshkm
