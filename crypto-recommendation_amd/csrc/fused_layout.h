// fused_layout.h — the one statement of the fused assignment's form rules and
// of its workspace: which shapes each form runs, the per-block list segments
// and their counters, and every buffer's size and regions. Plain host
// arithmetic: no HIP (tests/fused_layout_check.cpp includes it as it is).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace lshkm {

// ---- launch shapes the list capacity depends on (waves per block)
constexpr int FP_WAVES = 8;          // refinement: 2 waves per SIMD, the exact row kept in registers (<= 256 VGPRs)
constexpr int FH_WAVES_MIN = 8, FH_WAVES_MAX = 12;   // fh_waves() over all instantiations
constexpr int HMF_W = 4;             // hash_mfma_kernel
constexpr int HMF_BPC = 2;           // ... and its blocks per CU
constexpr int FP_KMAX = 256;         // centroids per refinement pass (hi + lo images in LDS)
constexpr int FH_KMAX = 512;         // centroids per hi-only pass (hi image only)
constexpr int FUSED_DIMS = 128;      // FU_D (tile.h)

// ---- the forms. hi: the hi-only passes, the refinement of the rows they list
// and the fix-ups; chunked: the streaming form (euclidean fp32 rows of 128
// dims: hashing with k != 4, and the tests' switch). rows: 0 = fp32 rows of
// 128 dims, 1 / 2 = general fp32 / fp64 rows of d <= 128 zero-padded dims (no
// hashing, K <= FH_KMAX). Hashing holds <= 32 functions per row; cosine
// hashing needs k = 4.
enum class FusedForm { none, hi, chunked };
struct FusedRoute {
    FusedForm form;
    int rows;
};
inline FusedRoute fused_route(bool cosine, bool f64, int d, int K, bool hash, int k, int LK, bool chunked_switch) {
    const bool hash_ok = !hash || (LK >= 1 && LK <= 32 && (!cosine || k == 4));
    if (!f64 && d == FUSED_DIMS && hash_ok) {
        if (!cosine) return {chunked_switch || (hash && k != 4) ? FusedForm::chunked : FusedForm::hi, 0};
        if (!chunked_switch) return {FusedForm::hi, 0};
    }
    if (!hash && d >= 1 && d <= FUSED_DIMS && K <= FH_KMAX) return {FusedForm::hi, f64 ? 2 : 1};
    return {FusedForm::none, 0};
}

// ---- lists. A kernel's block b owns segment b of each list it writes:
// entries [b * seg_rows, (b + 1) * seg_rows). Every counter buffer holds
// SEG_SLOTS int32 per segment for FUSED_MAX_SEGS segments, the one segment
// capacity of every grid. The fused kernels count block b's rows in
// [SEG_SLOTS * b + SEG_ROWS] and the fix-up records of the u64 list beside
// them in [SEG_SLOTS * b + SEG_FIX]; hash_mfma_kernel, which writes one list,
// counts block b in [b] of the same buffer.
constexpr int FUSED_MAX_SEGS = 1024;
constexpr int SEG_ROWS = 0, SEG_FIX = 1, SEG_SLOTS = 2;
constexpr size_t SEG_COUNTER_BYTES = (size_t)FUSED_MAX_SEGS * SEG_SLOTS * 4;
// A grid of nblk blocks of W waves deals the 32-row tiles round-robin, so a
// block holds at most W * 32 * ceil(tiles / (nblk * W)) rows: nblk segments of
// that many entries fit N + FUSED_LIST_SLACK for every nblk <= FUSED_MAX_SEGS
// and W <= FH_WAVES_MAX.
constexpr int64_t FUSED_LIST_SLACK = 32 + (int64_t)FUSED_MAX_SEGS * FH_WAVES_MAX * 32;
inline int64_t fused_list_cap(int64_t N) { return N + FUSED_LIST_SLACK; }
inline int64_t seg_rows_for(int64_t N, int nblk, int W) {
    const int64_t ntiles = (N + 31) / 32;
    return (int64_t)W * 32 * ((ntiles + (int64_t)nblk * W - 1) / ((int64_t)nblk * W));
}
// the fused kernels: one block per CU; one segment size for every wave count
inline int fused_grid(int64_t N, int ncu) {
    const int64_t want = ((N + 31) / 32 + FP_WAVES - 1) / FP_WAVES;
    return (int)std::max<int64_t>(1, std::min<int64_t>(ncu, want));
}
inline int64_t fused_seg_rows(int64_t N, int nblk) {
    int64_t r = 0;
    for (const int W : {FP_WAVES, FH_WAVES_MIN, FH_WAVES_MAX}) r = std::max(r, seg_rows_for(N, nblk, W));
    return r;
}
inline int hash_mfma_grid(int64_t N, int ncu) {
    const int64_t want = ((N + 31) / 32 + HMF_W - 1) / HMF_W;
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)ncu * HMF_BPC, want));
}
inline int64_t hash_mfma_seg_rows(int64_t N, int nblk) { return seg_rows_for(N, nblk, HMF_W); }

// ---- pass state (K > FP_KMAX): each lane's (best, runner-up, tile) crosses
// the passes in a float4, FUSED_PART_BYTES_PER_ROW per row of a 32-row tile.
// The hi-only passes index it by the row's tile; the refinement by (segment,
// tile of the segment's list): slot b * (seg_rows / 32) + t.
constexpr int64_t FUSED_PART_BYTES_PER_ROW = 32;
inline int64_t fused_part_bytes(int64_t N) {
    const int64_t tiles = std::max<int64_t>((N + 31) / 32, (fused_list_cap(N) + 31) / 32 + FUSED_MAX_SEGS);
    return tiles * 32 * FUSED_PART_BYTES_PER_ROW;
}

// ---- device counters of one call (u64 each)
constexpr int CNT_AMBIG = 0;         // rows left to the listed exact pass
constexpr int CNT_HFIX = 1;          // hash fix-up records
constexpr int CNT_REFINED = 2;       // rows the hi-only passes left to the refinement
constexpr int CNT_CFIX = 3;          // cosine declines / pow fix-ups
constexpr int CNT_PAIR = 4;          // uncertified rows the refinement named both candidates of and decided itself
constexpr size_t FUSED_COUNTER_BYTES = 64, FUSED_COUNTER_CLEAR = 40;
constexpr size_t FUSED_CBOUND_BYTES = 32;      // FusedArgs::cbound: the centroid prep's maxima start from zero

// ---- the workspace of one fused assignment
struct FusedShape {
    int64_t N = 0;
    int d = FUSED_DIMS, K = 0;
    bool cosine = false;
    int rows = 0;                    // FusedRoute::rows
    bool hash = false;               // the LSH outputs come from this pass
    int LK = 0;
    bool fast = false;               // euclidean: the certified f32 winner distance
    bool image32 = false;            // the f32 centroid image (fast, or the K <= 256 gather)
    bool own_tuples = false;         // euclidean hashing and the caller gave no tuple buffer
    int Kpad() const { return (K + 63) / 64 * 64; }
    // exact euclidean distances: rows whose chain met an inexact square (glibc's
    // pow(x, 2) may differ from x*x) are listed for the fix-up
    bool pwfix() const { return !cosine && !fast; }
    // the single-pass euclidean refinement names the two candidates of the rows
    // it can (the multi-pass form carries no runner-up tile: all to list2)
    bool pairs() const { return !cosine && Kpad() <= FP_KMAX; }
};
struct FusedLayout {
    static constexpr size_t NONE = ~(size_t)0;
    int64_t list_cap = 0;
    int64_t part_bytes = 0;          // 0: no pass state (Kpad <= FP_KMAX)
    // bytes of each buffer (0: this shape does not use it)
    size_t c16 = 0;                  // [Ch: Kpad x 128 f16][Cl: the same] at 0 / cl_off
    size_t cconst = 0;               // [cbound: 8 f32][cnh: Kpad f32][nbv: Kpad f64] at 0 / cnh_off / nbv_off
    size_t list1 = 0, list2 = 0;     // int32 rows: the hi-only passes' list, the refinement's
    size_t seg1 = 0, seg2 = 0, seg3 = 0;   // segment counters of list1 + hfix, list2 + hfix2, cfix
    size_t counter = 0;
    size_t fix = 0;                  // u64 records, regions of list_cap entries at hfix_off / cfix_off / hfix2_off:
                                     // [hash fix-ups][cosine declines of the hi-only passes, or pow fix-ups]
                                     // [cosine declines of the refinement]
                                     // [pair rows of the euclidean refinement]
    size_t part = 0;
    size_t tuples = 0;
    size_t cf32 = 0;                 // [C32: Kpad x 128 f32][rn32: Kpad f32] at 0 / rn32_off
    size_t c64p = 0;                 // general rows of d < 128: [Kpad][128] zero-padded fp64 centroids
    size_t xn2 = 0;                  // cosine on fp64 rows: [N] sums of squares
    size_t cl_off = 0, cnh_off = 0, nbv_off = 0, rn32_off = 0;
    size_t hfix_off = NONE, cfix_off = NONE, hfix2_off = NONE, pair_off = NONE;
};
inline FusedLayout fused_layout(const FusedShape& q) {
    FusedLayout l;
    const size_t Kpad = (size_t)q.Kpad(), D = FUSED_DIMS;
    const bool pwfix = q.pwfix();
    l.list_cap = fused_list_cap(q.N);
    const size_t cap = (size_t)l.list_cap, rows1 = (size_t)std::max<int64_t>(q.N, 1);
    l.c16 = Kpad * D * 2 * 2;
    l.cl_off = Kpad * D * 2;
    l.cconst = (Kpad + 8) * 4 + Kpad * 8;
    l.cnh_off = 8 * 4;
    l.nbv_off = (Kpad + 8) * 4;      // Kpad % 64 == 0: 8-byte aligned
    l.list1 = l.list2 = cap * 4;
    l.seg1 = l.seg2 = SEG_COUNTER_BYTES;
    l.counter = FUSED_COUNTER_BYTES;
    size_t regions = 0;
    if (q.hash || q.cosine || pwfix) regions++;      // region 0 is the hash fix-ups' in every shape that has a list
    if (q.hash || q.cosine) l.hfix_off = 0;
    if (q.cosine || pwfix) l.cfix_off = regions++ * cap * 8;
    if (q.cosine) l.hfix2_off = regions++ * cap * 8;
    if (q.pairs()) l.pair_off = regions++ * cap * 8;
    l.fix = regions * cap * 8;
    if (q.cosine || pwfix) l.seg3 = SEG_COUNTER_BYTES;
    if (Kpad > (size_t)FP_KMAX) l.part = (size_t)(l.part_bytes = fused_part_bytes(q.N));
    if (q.hash && !q.cosine && q.own_tuples) l.tuples = rows1 * (size_t)q.LK * 4;
    if (q.image32) {
        l.cf32 = Kpad * D * 4 + Kpad * 4;
        l.rn32_off = Kpad * D * 4;
    }
    if (q.rows != 0 && q.d != FUSED_DIMS) l.c64p = Kpad * D * 8;
    if (q.cosine && q.rows == 2) l.xn2 = rows1 * 8;
    return l;
}

// ---- the MFMA hashing on its own (hash_rows): one u64 list in the `fix`
// buffer, its counters in `seg1`, and the tuples when the caller keeps none
struct HashLayout {
    int64_t list_cap = 0;
    size_t fix = 0, seg1 = 0, tuples = 0;
};
inline HashLayout hash_layout(int64_t N, int LK, bool own_tuples) {
    HashLayout l;
    l.list_cap = fused_list_cap(N);
    l.fix = (size_t)l.list_cap * 8;
    l.seg1 = SEG_COUNTER_BYTES;
    if (own_tuples) l.tuples = (size_t)N * (size_t)LK * 4;
    return l;
}

}  // namespace lshkm
