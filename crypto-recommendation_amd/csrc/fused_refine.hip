// fused_refine.hip — the 3-product refinement of the fused pass (fused.hip):
// the rows a hi-only pass (fused_hi.hip) could not certify, scored again with
// the full split x = xh + xl, c = ch + cl.
#include "fused_impl.h"
#include "settle.h"

namespace lshkm {

// split8 in 2 VALU per element: v_cvt_pk_f16_f32 (hi pair), two residuals by
// v_fma_mix_f32, v_cvt_pk_f16_f32 (lo pair).
__device__ inline void split8p(const float* x, half8& hi, half8& lo) {
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const half2v hp = {(_Float16)x[j], (_Float16)x[j + 1]};
        hi[j] = hp.x;
        hi[j + 1] = hp.y;
        const half2v lp = {(_Float16)resid_lo(x[j], hp), (_Float16)resid_hi(x[j + 1], hp)};
        lo[j] = lp.x;
        lo[j + 1] = lp.y;
    }
}

// Scores of one 32-centroid tile: t = (hi + lo) + (-|c|^2/2) on packed f32
// (D rows of registers 4g..4g+3 are centroids 8g+4h..+3 of the tile).
__device__ inline void tile_scores(const floatx16& acc_hi, const floatx16& acc_lo, const float* cn_tile_h,
                                   float (&sv)[16]) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const float4 cn = *reinterpret_cast<const float4*>(cn_tile_h + 8 * g);
        const float2v h01 = {acc_hi[4 * g], acc_hi[4 * g + 1]}, l01 = {acc_lo[4 * g], acc_lo[4 * g + 1]};
        const float2v h23 = {acc_hi[4 * g + 2], acc_hi[4 * g + 3]}, l23 = {acc_lo[4 * g + 2], acc_lo[4 * g + 3]};
        const float2v c01 = {cn.x, cn.y}, c23 = {cn.z, cn.w};
        const float2v s01 = (h01 + l01) + c01, s23 = (h23 + l23) + c23;
        sv[4 * g] = s01.x; sv[4 * g + 1] = s01.y; sv[4 * g + 2] = s23.x; sv[4 * g + 3] = s23.y;
    }
}

__host__ __device__ constexpr int fp_lds_bytes(int Kpad) { return 16 + 2 * Kpad * FU_RS * 2 + Kpad * 4; }
static_assert(fp_lds_bytes(FP_KMAX) <= 160 * 1024, "refinement LDS image exceeds 160 KiB");
static_assert(FP_KMAX <= 32 * ST_TILES, "a settled row's candidate mask covers one refinement pass");

// ---- the pair rows' finish. A block decides its own pair rows before it ends,
// in the LDS its centroid image leaves behind: a wave takes FP_PAIR_REC records
// of the block's segment at a time, stages their rows (8 rows' values in flight
// at once, as the pruned pass loads its group), and two adjacent lanes per
// record run the two chains, the even lane on I1 and the odd one on I2. The pick
// between the two is the pruned pass's own (pruned_pick_euclid, pick.h), so
// argmin and distance are what that pass gives these rows. (As a kernel of its
// own after the refinement this waited for the hash fix-up's blocks, which fill
// every SIMD's registers, to end: DESIGN.md §9.)
constexpr int FP_PAIR_REC = 16;
constexpr int FP_PAIR_RS = FU_D | 1;     // odd row stride: element j of the staged rows in different banks
__host__ __device__ constexpr int fp_pair_lds_bytes(int rows) {
    return 16 + FP_WAVES * FP_PAIR_REC * FP_PAIR_RS * (rows == 2 ? 8 : 4);
}
static_assert(fp_pair_lds_bytes(2) <= 160 * 1024, "pair staging exceeds 160 KiB");
__host__ __device__ inline unsigned long long pair_record(int64_t row, int i1, int i2) {
    return (unsigned long long)(uint32_t)row | ((unsigned long long)(uint32_t)i1 << 32) |
           ((unsigned long long)(uint32_t)i2 << 48);
}
template <int ROWS>
__device__ inline void pair_finish(const FusedArgs& a, const unsigned long long* recs, int total, char* lds,
                                   int wave, int lane) {
    using TX = std::conditional_t<ROWS == 2, double, float>;
    const TX* X;
    if constexpr (ROWS == 2) X = a.X64; else X = a.X;
    const int d = ROWS == 0 ? FU_D : a.d;
    TX* xs = reinterpret_cast<TX*>(lds) + wave * FP_PAIR_REC * FP_PAIR_RS;
    for (int base = wave * FP_PAIR_REC; base < total; base += FP_WAVES * FP_PAIR_REC) {
        const int i = base + (lane >> 1);
        const unsigned long long rec = recs[min(i, total - 1)];
        int64_t row = (int64_t)(uint32_t)rec;
        int c = (lane & 1) ? (int)(rec >> 48) : (int)((rec >> 32) & 0xFFFFu);
        // lanes past the step's records, and a record that names nothing real, sit out
        if (lane >= 2 * FP_PAIR_REC || i >= total || row >= a.N) row = -1;
        if (row < 0 || c >= a.K) c = -1;
#pragma unroll 1
        for (int r0 = 0; r0 < FP_PAIR_REC && base + r0 < total; r0 += 8) {
            TX xv[8][FU_D / 64];
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int64_t rr = __shfl(row, 2 * (r0 + r));
#pragma unroll
                for (int u = 0; u < FU_D / 64; u++) {
                    const int j = lane + 64 * u;
                    xv[r][u] = j < d && rr >= 0 ? X[rr * d + j] : TX(0);
                }
            }
#pragma unroll
            for (int r = 0; r < 8; r++)
#pragma unroll
                for (int u = 0; u < FU_D / 64; u++) xs[(r0 + r) * FP_PAIR_RS + lane + 64 * u] = xv[r][u];
        }
        wave_sync();
        double best = 0.0;
        int bi = -1;
        pruned_pick_euclid<2>(xs + ((lane >> 1) & (FP_PAIR_REC - 1)) * FP_PAIR_RS, a.Cd, d, c, !a.fast_dist, best, bi);
        if (!(lane & 1) && bi >= 0) {
            a.assign[row] = bi;
            a.dist[row] = best;
        }
        wave_sync();
    }
}

// ---- the rows that are neither certified nor pair rows, settled by the wave
// that meets them (a.settle), so the call launches no listed pass. The tile's
// centroid tiles run once more and every lane keeps, per score, whether it
// reaches the certificate's own threshold M1 - 2E (settle.h's mask; the row's
// two lanes hold its set).
// The set contains the reference's nearest centroid, by the certificate's
// argument: E bounds |s - t| for every computed score s of the row against its
// true score t = x.c - |c|^2/2, for the plain f32 value tile_scores returns as
// for the value with the in-tile index packed into its low mantissa bits (the
// packing's 16 ulp are one of E's terms), and it covers the reference's own
// rounding of its distances (the 2^-41 |x|^2 term). M1 is the packed score of
// I1, so t_I1 >= M1 - E; a centroid whose plain score lies below M1 - 2E has
// t < M1 - E <= t_I1 by more than the reference can round away: it is neither
// the reference's nearest nor tied with it. The collecting pass compares the
// plain scores (the certificate compares packed ones; either is within E).
// Padding centroids (>= K) are dropped from the set.
// The rows are then taken one at a time by the whole wave, as the listed pruned
// pass's wave_decide takes them: at most 64 candidates, lane k runs the chain
// of the k-th (pruned_pick_euclid, the row read from global memory); more, or a
// row or centroid set outside the f16 range guard (no certificate: ok false),
// every centroid with the reference's chain. Any superset of the reference's
// near-ties gives the same pick: the chains are exact and the lowest index wins.
template <int ROWS>
__device__ inline void settle_rows(const FusedArgs& a, unsigned long long amask, const LaneMask& cand, int64_t row,
                                   bool ok, int lane) {
    using TX = std::conditional_t<ROWS == 2, double, float>;
    const TX* X;
    if constexpr (ROWS == 2) X = a.X64; else X = a.X;
    const int d = ROWS == 0 ? FU_D : a.d;
    for (unsigned long long m = amask; m; m &= m - 1) {      // wave-uniform: the rows' upper lanes
        const int up = __builtin_ctzll(m), lw = up - 32;
        const int64_t r = __shfl(row, up);
        const LaneMask m0 = {__shfl(cand.lo, lw), __shfl(cand.hi, lw)}, m1 = {__shfl(cand.lo, up), __shfl(cand.hi, up)};
        const bool rok = __shfl(ok ? 1 : 0, up) != 0;
        unsigned long long cm[ST_CHUNKS];
        const int n = settle_set(m0, m1, a.K, cm);
        const TX* xr = X + r * d;
        double best = 0.0;
        int bi = -1;
        if (rok && n >= 1 && n <= 64)
            pruned_pick_euclid<64>(xr, a.Cd, d, kth_candidate(cm, lane), !a.fast_dist, best, bi);
        else
            every_centroid(a.K, [&](int c) { return exact_euclid_rolled(xr, a.Cd + (size_t)c * d, d); }, best, bi);
        wave_store(best, bi, r, a.assign, a.dist);
    }
}

// For Kpad <= 256 the whole split centroid set (2 x 256 x 272 B) fits in LDS,
// so one block per CU loads it ONCE and its 8 waves (2 per SIMD) then loop
// independently over 32-row tiles: no barrier in the main loop, rows go
// straight from HBM into registers (lane half h: dims 16s+8h..+7 of row
// lane&31 -- the B-operand layout) and stay there, exact, for the winner's
// reference-order distance. Block b's rows are segment b of the list a hi-only
// pass wrote (a.list_in, counts in a.list_counts); the rows it cannot certify
// either go to the exact pass (a.ambig, segment b) -- or, euclidean and one
// pass, where the runner-up can be named and every third score lies below the
// certificate's window, to the block's pair segment (a.pairs), which the block
// decides itself after its last tile (pair_finish).
// MET = 1: cosine Lloyd: centroids are normalised in the prep (score x.c/|c|,
// cnh = 0), the winner distance is exact.h's certified form; declines are
// listed in a.hfix for the distance fix-up.
// MP: multi-pass (K > 256) form; the single-pass instantiation compiles without
// the pass-state code.
// ROWS = 1 / 2: the refinement of fused_hi_kernel<..., ROWS>'s rows (general
// rows, see there); fp64 rows add |x - f32(x)| |c| <= 2^-24 |x| |c| to E.
template <int MET, bool MP, int ROWS>
__global__ __launch_bounds__(FP_THREADS, 1) void fused_persistent_kernel(FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Kpad = a.Kpad;
    // euclidean, one pass: the runner-up is named too (tile_epilogue3), and an
    // uncertified row with every third score below the window is a pair row
    constexpr bool PAIR = MET == 0 && !MP;
    int* lcount = reinterpret_cast<int*>(smem);          // [0] ambiguous rows, [1] cosine declines / pair rows
    _Float16* lch = reinterpret_cast<_Float16*>(smem + 16);
    _Float16* lcl = lch + Kpad * FU_RS;
    float* lcn = reinterpret_cast<float*>(lcl + Kpad * FU_RS);

    // ---- prologue: the block's resident image (once per block), FP_CU granules
    // per thread in flight at once (a plain copy loop waited on every load)
    constexpr int FP_CU = 4;
    for (int e0 = 0; e0 < Kpad * 16; e0 += FP_THREADS * FP_CU) {
        float4 vh[FP_CU], vl[FP_CU];
#pragma unroll
        for (int u = 0; u < FP_CU; u++) {
            // past the end: granule 0 again (the same bytes rewritten), so neither
            // the loads nor the stores carry a branch and the loads issue together
            const int e = e0 + u * FP_THREADS + (int)threadIdx.x < Kpad * 16 ? e0 + u * FP_THREADS + (int)threadIdx.x : 0;
            const int r = e >> 4, g = e & 15;
            vh[u] = *reinterpret_cast<const float4*>(a.Ch + (size_t)r * FU_D + g * 8);
            vl[u] = *reinterpret_cast<const float4*>(a.Cl + (size_t)r * FU_D + g * 8);
        }
#pragma unroll
        for (int u = 0; u < FP_CU; u++) {
            const int e = e0 + u * FP_THREADS + (int)threadIdx.x < Kpad * 16 ? e0 + u * FP_THREADS + (int)threadIdx.x : 0;
            const int r = e >> 4, g = e & 15;
            *reinterpret_cast<float4*>(lch + r * FU_RS + g * 8) = vh[u];
            *reinterpret_cast<float4*>(lcl + r * FU_RS + g * 8) = vl[u];
        }
    }
    for (int e = threadIdx.x; e < Kpad; e += FP_THREADS) lcn[e] = a.cnh[e];
    if (threadIdx.x < 2) lcount[threadIdx.x] = 0;
    // This block's list segments (no device-wide atomic in the loop: a contended
    // global counter serialises at ~12 ns per add, MI355X_MICROARCH.md "fanin").
    int32_t* ambig_seg = a.ambig + (int64_t)blockIdx.x * a.seg_rows;
    unsigned long long* hfix_seg = a.hfix + (int64_t)blockIdx.x * a.seg_rows;
    unsigned long long* pair_seg = PAIR && a.pairs ? a.pairs + (int64_t)blockIdx.x * a.seg_rows : nullptr;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, h = lane >> 5;
    const float ecf = a.cbound[0], ebf = a.cbound[1], cmaxf = a.cbound[3];
    const bool c_ok = __float_as_uint(a.cbound[2]) == 0u;
    const _Float16* my_h = lch + col * FU_RS + 8 * h;
    const _Float16* my_l = lcl + col * FU_RS + 8 * h;
    const int ntile32 = Kpad >> 5;
    // this block's segment of the input list
    const int32_t* lrows = a.list_in + (int64_t)blockIdx.x * a.list_seg_rows;
    const int64_t lcnt = (int64_t)a.list_counts[SEG_SLOTS * blockIdx.x + SEG_ROWS];
    const int64_t ptile0 = (int64_t)blockIdx.x * ((a.list_seg_rows + 31) >> 5);   // part slots

    PT_DECL
    for (int64_t tile = wave; tile < (lcnt + 31) >> 5; tile += FP_WAVES) {
        const bool valid = tile * 32 + col < lcnt;
        const int64_t row = lrows[valid ? tile * 32 + col : lcnt - 1];
        const int64_t ptile = ptile0 + tile;      // pass-state slot

        // ---- point -> registers and the split B operand
        float xf[64];
        if constexpr (ROWS != 0) {
            load_row_gen<ROWS>(a, valid ? row : a.N - 1, h, xf);
        } else {
            // rows past N read row N-1 (results for them are never written)
            load_row_b(a.X + (valid ? row : a.N - 1) * FU_D + 8 * h, xf);
        }
        half8 bh[8], bl[8];
        float2v n2a = {0.f, 0.f}, n2b = {0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; s++) {
            split8p(xf + 8 * s, bh[s], bl[s]);
#pragma unroll
            for (int j = 0; j < 8; j += 4) {
                const float2v u = {xf[8 * s + j], xf[8 * s + j + 1]}, v = {xf[8 * s + j + 2], xf[8 * s + j + 3]};
                n2a = __builtin_elementwise_fma(u, u, n2a);
                n2b = __builtin_elementwise_fma(v, v, n2b);
            }
        }
        float xn2f = (n2a.x + n2a.y) + (n2b.x + n2b.y);
        xn2f += __shfl_xor(xn2f, 32);
        // f32 sum of squares: inflate by 2^-16 (> d 2^-24) to stay an upper bound;
        // |x|_1 <= sqrt(d) |x|_2 replaces the L1 norm in the A2 terms, and
        // |x|_2 <= 2^15 implies the f16 range guard |x_j| <= 2^15 (false for nan/inf).
        const double xn2 = (double)xn2f * (1.0 + 0x1p-16);
        const double nx = sqrt(xn2);
        const double x1 = FU_SQRT_D * nx;
        const bool x_ok = xn2f <= FU_RANGE * FU_RANGE;

        PT_MARK(0)
        PT_MARK(1)      // phase 1 was the hash tile: the phase numbers of the profiles stay
        // ---- all centroid tiles from the resident image
        // Each score carries its in-tile index (4g+q) in its low 4 mantissa bits:
        // a perturbation below 16 ulp <= 2^-19 |t|, |t| <= |x| cmax + cmax^2/2,
        // charged to E (with 2x margin). The running max then identifies the
        // winner without a compare/select per score; its tile is noted per tile.
        // cosine: |t| <= |x| |c^| (no -|c|^2/2 term); + 2^-43 |x| covers the
        // normalisation's roundings and the reference's own: its q = x.c / (|x||c|)
        // carries <= 2^-46 relative (the fp64 norm chains), and 1 - q rounds at 2^-52
        const float E = MET == 0
            ? (float)(nx * (double)ecf + (double)ebf + FU_A2 * x1 + 0x1p-41 * xn2 +
                      0x1p-18 * (nx * (double)cmaxf + 0.5 * (double)cmaxf * (double)cmaxf) +
                      (ROWS == 2 ? 0x1p-24 * nx * (double)cmaxf : 0.0)) * (1.f + 0x1p-20f) + 1e-30f
            : (float)(nx * (double)ecf + (double)ebf + FU_A2 * x1 + 0x1p-41 * xn2 +
                      0x1p-18 * nx * (double)cmaxf + 0x1p-43 * nx) * (1.f + 0x1p-20f) + 1e-30f;
        float m1 = -__builtin_inff(), m2 = -__builtin_inff();
        int t1 = 0;
        Top3 top = {m1, m1, m1, 0, 0};        // PAIR: the running state instead of (m1, m2, t1)
        if (MP && !a.pass_first) {
            const float4 st = a.part[ptile * 64 + lane];
            m1 = st.x; m2 = st.y; t1 = __float_as_int(st.z);
        }
        const int tg0 = MP ? a.t0 : 0;        // global index of this slice's first tile
        __builtin_amdgcn_s_setprio(MFMA_PRIO);
#pragma unroll 1
        for (int t = 0; t < ntile32; t++) {
            float sv[16];
            floatx16 acc_hi, acc_lo;
            tile_mfma(my_h + t * 32 * FU_RS, my_l + t * 32 * FU_RS, bh, bl, acc_hi, acc_lo);
            tile_scores(acc_hi, acc_lo, lcn + t * 32 + 4 * h, sv);
            if constexpr (PAIR) {
                tile_epilogue3(sv, t, top);
            } else {
                const float m1_prev = m1;
                tile_epilogue(sv, m1, m2);
                t1 = m1 != m1_prev ? t + tg0 : t1;
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (PAIR) { m1 = top.m1; m2 = top.m2; t1 = top.t1; }
        if (MP && !a.pass_last) {             // more slices to come: carry the state
            a.part[ptile * 64 + lane] = make_float4(m1, m2, __int_as_float(t1), 0.f);
            continue;
        }
        const uint32_t l1 = __float_as_uint(m1) & 0xFu;
        const int i1 = t1 * 32 + 8 * (int)(l1 >> 2) + 4 * h + (int)(l1 & 3u);
        const float om1 = __shfl_xor(m1, 32), om2 = __shfl_xor(m2, 32);
        const int oi1 = __shfl_xor(i1, 32);
        const float M2 = fmaxf(fmaxf(m2, om2), fminf(m1, om1));
        const int I1 = (om1 > m1 || (om1 == m1 && oi1 < i1)) ? oi1 : i1;
        const float M1 = fmaxf(m1, om1);
        const bool cert = x_ok && c_ok && ((double)M2 < (double)M1 - 2.0 * (double)E);
        // A pair row: not certified, but every score other than I1's and I2's is
        // below the same window (M3 bounds them all), so no third centroid can be
        // the reference's nearest or tie with it: {I1, I2} decides the row.
        bool pair = false;
        int I2 = 0;
        if constexpr (PAIR) {
            const uint32_t l2 = __float_as_uint(m2) & 0xFu;
            const int i2 = top.t2 * 32 + 8 * (int)(l2 >> 2) + 4 * h + (int)(l2 & 3u);
            const HalfTop me = {m1, m2, top.m3, i1, i2};
            const HalfTop ot = {om1, om2, __shfl_xor(top.m3, 32), oi1, __shfl_xor(i2, 32)};
            const PairMerge pm = I1 == i1 ? merge_halves(me, ot) : merge_halves(ot, me);
            I2 = pm.I2;
            pair = pair_seg && !cert && x_ok && c_ok && I1 != I2 && I1 < a.K && I2 < a.K &&
                   (double)pm.M3 < (double)M1 - 2.0 * (double)E;
        }

        // A row nobody else decides: with a.settle the wave decides it below, from
        // the candidates a second run of the tile's centroid tiles collects here,
        // while the split operand is still in registers (wave-uniform branch)
        const bool amb = valid && !cert && !pair;
        LaneMask cand = {0ull, 0ull};
        bool settle = false;
        if constexpr (PAIR) {
            settle = a.settle && __ballot(amb) != 0ull;
            if (settle) {
                const double thr = (double)M1 - 2.0 * (double)E;
                __builtin_amdgcn_s_setprio(MFMA_PRIO);
#pragma unroll 1
                for (int t = 0; t < ntile32; t++) {
                    float sv[16];
                    floatx16 acc_hi, acc_lo;
                    tile_mfma(my_h + t * 32 * FU_RS, my_l + t * 32 * FU_RS, bh, bl, acc_hi, acc_lo);
                    tile_scores(acc_hi, acc_lo, lcn + t * 32 + 4 * h, sv);
                    uint32_t bits = 0u;
#pragma unroll
                    for (int i = 0; i < 16; i++) bits |= (double)sv[i] >= thr ? 1u << i : 0u;
                    settle_mark(cand, t, bits);
                }
                __builtin_amdgcn_s_setprio(0);
            }
        }

        // ---- winner distance in reference order: the squares are independent,
        // only the sum is a chain; dims 8seg..8seg+7 belong to lane half seg & 1,
        // and the halves hand the sum on after every 8 dims.
        PT_MARK(2)
        if constexpr (MET == 1) {
            // cosine winner: one lane per point re-reads its row (L2) and the
            // winner's fp64 row; declined certificates -> the fix-up list
            bool fix = false;
            if (h == 1 && valid && cert) {
                a.assign[row] = I1;
                double v;
                bool okc;
                if constexpr (ROWS == 1) okc = cosine_fast_nb(a.X + row * a.d, a.Cd + (size_t)I1 * a.d, a.d, a.nbv[I1], v);
                else if constexpr (ROWS == 2) okc = cosine_fast_nb(a.X64 + row * a.d, a.Cd + (size_t)I1 * a.d, a.d, a.nbv[I1], v);
                else okc = cosine_fast_nb(a.X + row * FU_D, a.C64 + (size_t)I1 * FU_D, FU_D, a.nbv[I1], v);
                if (okc) a.dist[row] = v;
                else fix = true;
            }
            const unsigned long long fb = __ballot(fix);
            if (fb) {
                const int leader = __builtin_ctzll(fb);
                int base = 0;
                if (lane == leader) base = atomicAdd(lcount + 1, __popcll(fb));
                base = __shfl(base, leader);
                if (fix) hfix_seg[base + __popcll(fb & ((1ull << lane) - 1ull))] = (unsigned long long)row;
            }
        } else {
            // exact row still in registers (B-operand layout): lane half h owns
            // dims 16s+8h..+7; only the winner's fp64 row is loaded, one 16-dim
            // step ahead (deeper prefetch measured slower: DESIGN.md)
            const double* crow = a.C64 + (size_t)I1 * FU_D + 8 * h;
            double acc = 0.0;
            double2 cbuf[4];
            double2 xnext[4];                 // fp64 rows: the exact values, one step ahead
            const int64_t rowc = valid ? row : a.N - 1;
            if constexpr (ROWS == 2) load_x64_step(a, rowc, 0, h, xnext);
#pragma unroll
            for (int j = 0; j < 4; j++) cbuf[j] = *reinterpret_cast<const double2*>(crow + 2 * j);
#pragma unroll
            for (int s = 0; s < 8; s++) {
                double sq[8];
                double2 cur[4];
#pragma unroll
                for (int j = 0; j < 4; j++) cur[j] = cbuf[j];
                if (s + 1 < 8) {
#pragma unroll
                    for (int j = 0; j < 4; j++) cbuf[j] = *reinterpret_cast<const double2*>(crow + 16 * (s + 1) + 2 * j);
                }
                double2 xcur[4];
                if constexpr (ROWS == 2) {
#pragma unroll
                    for (int j = 0; j < 4; j++) xcur[j] = xnext[j];
                    if (s + 1 < 8) load_x64_step(a, rowc, s + 1, h, xnext);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) xcur[j] = make_double2((double)xf[8 * s + 2 * j], (double)xf[8 * s + 2 * j + 1]);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double2 cc = cur[j];
                    const double d0 = __dsub_rn(xcur[j].x, cc.x);
                    const double d1 = __dsub_rn(xcur[j].y, cc.y);
                    // LSHKM_DIST_CERTIFIED: x*x (the chain within 2^-44 of the
                    // reference's, inside the 2^-20 contract); exact: glibc's pow
                    sq[2 * j] = a.fast_dist ? __dmul_rn(d0, d0) : gp_sq(d0);
                    sq[2 * j + 1] = a.fast_dist ? __dmul_rn(d1, d1) : gp_sq(d1);
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
            if (h == 1 && valid && cert) {
                a.assign[row] = I1;
                a.dist[row] = sqrt(acc);
            }
        }
        PT_MARK(3)
        if constexpr (PAIR)
            seg_append(valid && pair && h == 1, pair_record(row, I1, I2), lcount + 1, pair_seg, lane);
        const unsigned long long amask = __ballot(amb && h == 1);
        if (h == 1 && valid) {
            if (amb) {
                int base = 0;
                const int leader = __builtin_ctzll(amask);
                if (lane == leader) base = atomicAdd(lcount, __popcll(amask));
                base = __shfl(base, leader);
                const int rank = __popcll(amask & ((1ull << lane) - 1ull));
                if (!(PAIR && a.settle)) ambig_seg[base + rank] = (int32_t)row;     // settled here: counted only
            }
        }
        if constexpr (PAIR) {
            if (settle) settle_rows<ROWS>(a, amask, cand, row, x_ok && c_ok, lane);
        }
        PT_MARK(4)
    }
    PT_FLUSH
    __syncthreads();
    // the block's pair rows, once every wave is done with the image (uniform: pair_seg, lcount)
    if constexpr (PAIR) {
        if (pair_seg && lcount[1] > 0) pair_finish<ROWS>(a, pair_seg, lcount[1], smem + 16, wave, lane);
    }
    // slot 0: ambiguous rows; slot 1: the cosine fix-up list, or the pair rows (the last pass decides both)
    if (threadIdx.x < 2 && (!MP || (threadIdx.x == 0 ? a.pass_last != 0 : (MET == 1 && a.pass_last)))) {
        const int c = lcount[threadIdx.x];
        a.seg_counts[SEG_SLOTS * blockIdx.x + threadIdx.x] = c;
        if (c) atomicAdd(threadIdx.x == 0 ? a.ambig_count : MET == 1 ? a.hfix_count : a.pair_count, (unsigned long long)c);
    }
}

template <int MET, bool MP, int ROWS>
static void refine_launch(hipStream_t s, unsigned nblk, const FusedArgs& a) {
    // the image, or the pair rows' staging where that is larger (few centroids)
    const int lds = MET == 0 && !MP && a.pairs ? std::max(fp_lds_bytes(a.Kpad), fp_pair_lds_bytes(ROWS)) : fp_lds_bytes(a.Kpad);
    hipLaunchKernelGGL((fused_persistent_kernel<MET, MP, ROWS>), dim3(nblk), dim3(FP_THREADS), (size_t)lds, s, a);
}
template <int MET, bool MP>
static void refine_rows(hipStream_t s, unsigned nblk, int rows, const FusedArgs& a) {
    if (rows == 0) refine_launch<MET, MP, 0>(s, nblk, a);
    else if (rows == 1) refine_launch<MET, MP, 1>(s, nblk, a);
    else refine_launch<MET, MP, 2>(s, nblk, a);
}

int launch_fused_refine_pass(hipStream_t s, unsigned nblk, int metric, bool mp, int rows, const FusedArgs& a) {
    if (metric < 0 || metric > 1 || rows < 0 || rows > 2 || a.Kpad > FP_KMAX) {
        set_error("launch_fused_refine_pass: no kernel for this metric / row kind / slice");
        return -1;
    }
    if (metric == 1) mp ? refine_rows<1, true>(s, nblk, rows, a) : refine_rows<1, false>(s, nblk, rows, a);
    else mp ? refine_rows<0, true>(s, nblk, rows, a) : refine_rows<0, false>(s, nblk, rows, a);
    return 0;
}

}  // namespace lshkm
