// fused.hip — one pass over the points: LSH hashing + Lloyd assignment on gfx950.
//
// Replaces, in one read of each point (SURVEY §8a rows a1-a3, a7's bucket ID,
// a12): EuclideanPhiGen::generate (lib/generators/euclidean_phi_gen.hpp:77-92)
// for L tables of k EuclideanH functions (euclidean_h_gen.hpp:73-76), and
// lloyds_assignment (lib/clustering_phases/assignment.hpp:54-80).
//
// Split-precision f16 MFMA. Every operand is split x = xh + xl (xh = f16(x),
// xl = f16(x - xh)); a dot product is sum(xh ch) [acc_hi] + sum(xh cl + xl ch)
// [acc_lo] on v_mfma_f32_32x32x16_f16: products of f16 values are exact in
// f32, and the separate hi accumulator keeps the rounding of the large terms
// at d ulps of f32. Rigorous bound on |dot~ - x.c|:
//   A1 |x||c| + A2 (|x|_1 + |c|_1),  A1 = 1.25 * 2^-16, A2 = 2^-24,
// which assumes nothing better than round-toward-zero accumulation. The f16
// range is guarded: a point with |x_j| > 2^15 (or non-finite) or a centroid set
// with |c_j| > 2^15 is never certified, so such inputs take the exact path.
//
// This file is the launch sequence alone; the kernels live in fused_hi.hip
// (scores from the hi products only: most rows are certified there),
// fused_refine.hip (the 3-product refinement of the rows it lists),
// fused_small.hip (centroid prep and the fix-ups) and fused_chunked.hip (the
// streaming form for k != 4), and fused_impl.h holds what they share.
#include "fused_impl.h"

namespace lshkm {

namespace {

// What a launch works out once: the grid (one block per CU) and the forms.
struct FusedPlan {
    bool hash = false, cos = false;
    int nblk = 0;
    int np_hi = 0;       // hi-only passes (FH_KMAX centroids each)
    int np_refine = 0;   // refinement passes (FP_KMAX centroids each)
    bool side = false;   // the hash fix-up runs on the side stream
};

int fused_validate(bool hash, const FusedLaunch& f, const FusedArgs& a, bool chunked, bool multi_ok, int npass) {
    if (f.rows != 0 && (hash || a.Kpad > FH_KMAX || f.a.d < 1 || f.a.d > FU_D || (f.metric == 1 && !a.Cd) ||
                        (f.rows == 1 ? !a.X : (f.rows != 2 || !a.X64)))) {
        set_error("launch_fused: general rows run the hi-only form without hashing, K <= 512, d <= 128");
        return -1;
    }
    // refinement pass state: one slot per (segment, tile) of the list
    if (npass > 1 && f.part_bytes < ((f.list_cap + 31) / 32 + FUSED_MAX_SEGS) * 64 * 16) {
        set_error("launch_fused: pass-state buffer too small for the refinement");
        return -1;
    }
    if (f.metric == 1 && (chunked || !multi_ok || !a.nbv || !a.hfix || !a.hfix_count || (hash && a.k != 4))) {
        set_error("launch_fused: cosine runs the hi-only form only (hashing: k = 4)");
        return -1;
    }
    if (f.metric == 1 && f.rows == 2 && !a.xn2) {
        set_error("launch_fused: cosine on fp64 rows needs the rows' sums of squares");
        return -1;
    }
    if ((f.metric == 1 || !a.fast_dist) && (!a.cfix || !a.cfix_counts || !a.cfix_count)) {
        set_error("launch_fused: the hi-only cosine form needs the decline list, the exact euclidean one the pow fix-up list");
        return -1;
    }
    if (hash && (a.LK > 32 || a.L * a.k != a.LK)) {              // the fix-ups hold <= 32 functions per row
        set_error("launch_fused: hashing needs L * k <= 32");
        return -1;
    }
    return 0;
}

// One block per CU; the lists' segment size; the workspace checks.
int fused_plan(bool hash, FusedLaunch& f, FusedArgs& a, FusedPlan& p) {
    int ncu = 0;
    if (device_cu_count(&ncu)) return -2;
    const int64_t ntiles = (a.N + 31) / 32;
    const int64_t want = (ntiles + FP_WAVES - 1) / FP_WAVES;
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(ncu, want));
    // list segments: block b's tiles hold at most W * 32 * ceil(tiles / (grid * W))
    // rows, for every wave count W a kernel may run with
    a.seg_rows = 0;
    for (const int W : {FP_WAVES, FH_WAVES_MIN, FH_WAVES_MAX})
        a.seg_rows = std::max<int64_t>(a.seg_rows, (int64_t)W * 32 * ((ntiles + (int64_t)nblk * W - 1) / ((int64_t)nblk * W)));
    a.seg_counts = f.seg_counts;
    if (!f.seg_counts || f.seg_cap < nblk || (int64_t)nblk * a.seg_rows > f.list_cap) {
        set_error("launch_fused: list workspace too small");
        return -1;
    }
    f.nseg = nblk;
    f.seg_rows = a.seg_rows;
    if (hash && (!a.hfix || !a.hfix_count || (f.metric == 0 && !a.tuples) || a.LKpad > 32)) {   // pts[] holds 128 x 32 projections
        set_error("launch_fused: hashing needs the fix-up list, a tuple buffer and L*k <= 32");
        return -1;
    }
    if (!f.list2 || !f.seg_counts2 || !f.refined || (f.a.Kpad > FH_KMAX && !f.part) || (f.metric == 1 && !f.hfix2)) {
        set_error("launch_fused: the hi-only form needs the second list and its counters");
        return -1;
    }
    p.hash = hash;
    p.cos = f.metric == 1;
    p.nblk = nblk;
    p.np_hi = (f.a.Kpad + FH_KMAX - 1) / FH_KMAX;
    p.np_refine = (f.a.Kpad + FP_KMAX - 1) / FP_KMAX;
    p.side = hash && f.side && f.fork && f.join;
    return 0;
}

// The hi-only passes over all rows; the rows they cannot certify go to a.ambig.
int fused_hi_passes(hipStream_t s, const FusedLaunch& f, FusedArgs& a, const FusedPlan& p) {
    const bool gather_on = !test_switch("LSHKM_GATHER", "0");
    int rc;
    if (f.rows != 0) {
        // general rows: one pass (Kpad <= 512)
        HiForm h;
        h.metric = f.metric; h.rows = f.rows;
        h.fast = !p.cos && a.fast_dist;
        h.gath = !p.cos && !h.fast && f.rows == 1 && a.Kpad <= FH_GATH_KMAX && gather_on;
        return launch_fused_hi_pass(s, p.nblk, h, a);
    }
    // 512 < K <= 1024, euclidean, LSHKM_HI_TWO_IMAGE=1: one two-image launch
    // instead of two passes with carried state. Measured at C5 (N = 10M,
    // K = 1024): 5.09 ms vs 1.83 + 2.51 ms, HBM 8.9 GB vs 13.8 GB per call --
    // the block-wide image swaps line the waves up and cost the MFMA/VALU
    // overlap between them, more than the second read of X costs; opt-in.
    if (!p.cos && p.np_hi == 2 && test_switch("LSHKM_HI_TWO_IMAGE", "1")) {
        HiForm h;
        h.hash = p.hash; h.two_image = true;
        return launch_fused_hi_pass(s, p.nblk, h, a);
    }
    for (int i = 0; i < p.np_hi; i++) {
        const int c0 = i * FH_KMAX;
        a.Ch = f.a.Ch + (size_t)c0 * FU_D; a.cnh = f.a.cnh + c0;
        a.Kpad = std::min(FH_KMAX, f.a.Kpad - c0);
        a.t0 = c0 / 32; a.pass_first = i == 0; a.pass_last = i == p.np_hi - 1;
        HiForm h;
        h.hash = p.hash && i == 0; h.mp = p.np_hi > 1; h.metric = f.metric;
        if (!p.cos && !h.mp) {
            // K <= 256: the certified f32 winner distance compiled in, else the
            // winner rows by the LDS-DMA gather (LSHKM_GATHER=0: register loads)
            const bool small = a.Kpad <= FH_GATH_KMAX && gather_on;
            h.fast = small && a.fast_dist;
            h.gath = small && !a.fast_dist;
        } else if (!p.cos) {
            h.fast = !h.hash && a.fast_dist && a.pass_last;
        }
        if ((rc = launch_fused_hi_pass(s, p.nblk, h, a))) return rc;
    }
    return 0;
}

// The hash fix-up touches only tuples / phi / bucket of its listed rows: on
// the side stream beside the refinement when one is given.
int fused_hash_fixup(hipStream_t s, FusedLaunch& f, const FusedArgs& a, const FusedPlan& p) {
    hipStream_t hs = p.side ? f.side : s;
    if (p.side) {
        if (hipEventRecord(f.fork, s) != hipSuccess || hipStreamWaitEvent(f.side, f.fork, 0) != hipSuccess)
            return kstatus("launch_fused (fork)");
    }
    if (p.hash) launch_hash_fixup(hs, (unsigned)p.nblk, p.cos, a);
    if (p.side && f.side_timing) {
        if (hipEventRecord(f.side_timing, f.side) != hipSuccess) {
            (void)hipStreamSynchronize(f.side);
            return kstatus("launch_fused (timing)");
        }
        f.side_timed = true;
    }
    if (p.side && hipEventRecord(f.join, f.side) != hipSuccess) {
        // never return with the fix-up unordered against later work on s
        (void)hipStreamSynchronize(f.side);
        return kstatus("launch_fused (join)");
    }
    return 0;
}

// The 3-product refinement of the rows in a.ambig, FP_KMAX centroids per pass;
// what it cannot certify goes to list2 for the caller's exact pass.
int fused_refine_passes(hipStream_t s, const FusedLaunch& f, const FusedArgs& a, const FusedPlan& p) {
    FusedArgs r = a;
    r.list_in = a.ambig; r.list_counts = f.seg_counts; r.list_seg_rows = a.seg_rows;
    r.ambig = f.list2; r.seg_counts = f.seg_counts2; r.ambig_count = f.a.ambig_count;
    r.hfix = p.cos ? f.hfix2 : f.a.hfix; r.hfix_count = p.cos ? f.a.cfix_count : f.a.hfix_count;
    r.tuples = nullptr; r.phi = nullptr; r.bucket = nullptr;
    for (int i = 0; i < p.np_refine; i++) {
        const int c0 = i * FP_KMAX;
        r.Ch = f.a.Ch + (size_t)c0 * FU_D; r.Cl = f.a.Cl + (size_t)c0 * FU_D; r.cnh = f.a.cnh + c0;
        r.Kpad = std::min(FP_KMAX, f.a.Kpad - c0);
        r.t0 = c0 / 32; r.pass_first = i == 0; r.pass_last = i == p.np_refine - 1;
        const int rc = launch_fused_refine_pass(s, (unsigned)p.nblk, f.metric, p.np_refine > 1, f.rows, r);
        if (rc) return rc;
    }
    return 0;
}

// out: the lists the caller still has to work through
void fused_output_lists(FusedLaunch& f, const FusedArgs& a, const FusedPlan& p) {
    f.final_list = f.list2;
    f.final_counts = f.seg_counts2;
    if (!p.cos && !a.fast_dist && a.cfix) {      // the hi-only pass's pow fix-ups (exact distances)
        f.ncos_lists = 1;
        f.cos_list[0] = a.cfix; f.cos_counts[0] = a.cfix_counts;
    }
    if (p.cos) {
        f.ncos_lists = 2;
        f.cos_list[0] = a.cfix; f.cos_counts[0] = a.cfix_counts;
        f.cos_list[1] = f.hfix2; f.cos_counts[1] = f.seg_counts2;
    }
}

}  // namespace

int launch_fused(hipStream_t s, bool hash, FusedLaunch& f) {
    f.nseg = 0;
    f.side_timed = false;
    if (f.a.N <= 0) return 0;
    // the caller's block, then the fields this launch derives
    FusedArgs a = f.a;
    a.bdiv = make_bucket_div(a.nb);
    a.part = nullptr; a.t0 = 0; a.pass_first = 1; a.pass_last = 1;
    a.list_in = nullptr; a.list_counts = nullptr; a.list_seg_rows = 0;
    a.prof = nullptr;
    a.pw_lds = 0;
    a.fast_dist = f.a.fast_dist && f.metric == 0 && f.rows != 2 && a.C32 && a.rn32 ? 1 : 0;
    a.d = f.rows == 0 ? FU_D : f.a.d;
    a.xvec = f.rows == 1 ? (a.d % 4 == 0 && ((uintptr_t)a.X & 15) == 0)
                         : (a.d % 2 == 0 && ((uintptr_t)a.X64 & 15) == 0);
#ifdef LSHKM_PHASE_TIMING
    static unsigned long long* prof_d = nullptr;
    if (!prof_d) (void)hipMalloc(&prof_d, 64);
    (void)hipMemsetAsync(prof_d, 0, 64, s);
    a.prof = prof_d;
    struct PhaseReport {      // printed after the launch sequence below
        hipStream_t s; unsigned long long* d;
        ~PhaseReport() {
            unsigned long long v[6];
            (void)hipMemcpyAsync(v, d, 48, hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            // hi-only form: [0] load + split + hash, [1] centroid tiles, [2] certificate + chain + stores
            // (the refinement's fused_persistent_kernel adds its own phases 0-4 over its few rows)
            fprintf(stderr, "PHASES %llu %llu %llu %llu %llu\n", v[0], v[1], v[2], v[3], v[4]);
        }
    } report{s, prof_d};
#endif
    const bool chunked = test_switch("LSHKM_FUSED_FORM", "chunked") && f.rows == 0;   // the streaming form (tests)
    const int npass = (a.Kpad + FP_KMAX - 1) / FP_KMAX;
    const bool multi_ok = npass == 1 || (f.part && f.part_bytes >= ((a.N + 31) / 32) * 64 * 16);
    int rc;
    if ((rc = fused_validate(hash, f, a, chunked, multi_ok, npass))) return rc;
    if (chunked || !multi_ok || (hash && a.k != 4)) return launch_fused_chunked(s, hash, a);

    FusedPlan p;
    if ((rc = fused_plan(hash, f, a, p))) return rc;
    a.part = reinterpret_cast<float4*>(f.part);
    a.ambig_count = f.refined;
    if ((rc = fused_hi_passes(s, f, a, p))) return rc;
    if ((rc = fused_hash_fixup(s, f, a, p))) return rc;
    if ((rc = fused_refine_passes(s, f, a, p))) {
        if (p.side) (void)hipStreamSynchronize(f.side);
        return rc;
    }
    fused_output_lists(f, a, p);
    if (p.side && f.defer_join) {
        f.join_pending = true;          // the caller joins (after its exact pass)
    } else if (p.side && hipStreamWaitEvent(s, f.join, 0) != hipSuccess) {
        (void)hipStreamSynchronize(f.side);
        return kstatus("launch_fused (join)");
    }
    return kstatus("fused_hi_kernel");
}

}  // namespace lshkm
