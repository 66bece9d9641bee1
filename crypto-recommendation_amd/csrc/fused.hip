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
//   A1 |x||c| + A2 (|x|_1 + |c|_1),  A1 = FU_A1 = 1.057 * 2^-16 (tile.h: the sum
// of its parts), A2 = 2^-24,
// which assumes nothing better than round-toward-zero accumulation. The f16
// range is guarded: a point with |x_j| > 2^15 (or non-finite) or a centroid set
// with |c_j| > 2^15 is never certified, so such inputs take the exact path.
//
// This file is the host side alone: fused_assign, from the workspace to the
// last fix-up. The kernels live in fused_hi.hip
// (scores from the hi products only: most rows are certified there),
// fused_refine.hip (the 3-product refinement of the rows it lists),
// fused_small.hip (centroid prep and the fix-ups) and fused_chunked.hip (the
// streaming form for k != 4), and fused_impl.h holds what they share.
#include "../../include/lshkm.h"
#include "fused_impl.h"
#include "index.h"

namespace lshkm {

namespace {

// What a call works out once: the grid (one block per CU), the lists' segment
// size and the passes.
struct FusedPlan {
    bool hash = false, cos = false;
    int rows = 0;
    int nblk = 0;
    int64_t seg_rows = 0;
    int np_hi = 0;       // hi-only passes (FH_KMAX centroids each)
    int np_refine = 0;   // refinement passes (FP_KMAX centroids each)
};

// The context's buffers at fused_layout's sizes, as typed pointers: the one
// place that names them (the allocation order is part of the contract: a
// buffer grows in place of its own earlier allocation only).
int fused_workspace(lshkm_ctx ctx, const FusedShape& sh, FusedWorkspace& w) {
    const FusedLayout l = fused_layout(sh);
    int rc;
    struct { Buf& b; size_t bytes; } const bufs[] = {
        {ctx->ws_c32, l.c16},      {ctx->ws_cconst, l.cconst}, {ctx->ws_ambig, l.list1}, {ctx->ws_counter, l.counter},
        {ctx->ws_seg, l.seg1},     {ctx->ws_hfix, l.fix},      {ctx->ws_seg3, l.seg3},   {ctx->ws_part, l.part},
        {ctx->ws_ambig2, l.list2}, {ctx->ws_seg2, l.seg2},     {ctx->ws_tuples, l.tuples}, {ctx->ws_cf32, l.cf32},
        {ctx->ws_c64p, l.c64p},    {ctx->ws_xn2, l.xn2}};
    for (const auto& e : bufs)
        if (e.bytes && (rc = e.b.reserve(e.bytes))) return rc;
    const auto at = [](const Buf& b, size_t off) { return off == FusedLayout::NONE ? nullptr : (char*)b.p + off; };
    w.list_cap = l.list_cap;
    w.Ch = (_Float16*)at(ctx->ws_c32, 0); w.Cl = (_Float16*)at(ctx->ws_c32, l.cl_off);
    w.cbound = (float*)at(ctx->ws_cconst, 0); w.cnh = (float*)at(ctx->ws_cconst, l.cnh_off);
    w.nbv = (double*)at(ctx->ws_cconst, l.nbv_off);
    if (l.cf32) { w.C32 = (float*)at(ctx->ws_cf32, 0); w.rn32 = (float*)at(ctx->ws_cf32, l.rn32_off); }
    if (l.c64p) w.C64p = ctx->ws_c64p.as<double>();
    w.list1 = ctx->ws_ambig.as<int32_t>(); w.seg1 = ctx->ws_seg.as<int32_t>();
    w.list2 = ctx->ws_ambig2.as<int32_t>(); w.seg2 = ctx->ws_seg2.as<int32_t>();
    if (l.seg3) w.seg3 = ctx->ws_seg3.as<int32_t>();
    w.hfix = (unsigned long long*)at(ctx->ws_hfix, l.hfix_off);
    w.cfix = (unsigned long long*)at(ctx->ws_hfix, l.cfix_off);
    w.hfix2 = (unsigned long long*)at(ctx->ws_hfix, l.hfix2_off);
    w.pairs = (unsigned long long*)at(ctx->ws_hfix, l.pair_off);
    if (l.part) w.part = ctx->ws_part.as<float4>();
    w.cnt = ctx->ws_counter.as<unsigned long long>();
    if (l.xn2) w.xn2 = ctx->ws_xn2.as<double>();
    if (l.tuples) w.tuples = ctx->ws_tuples.as<int32_t>();
    return 0;
}

// The kernels' argument block, from the request and the workspace: everything
// but the lists and the per-pass fields, which each stage sets for itself.
FusedArgs fused_common_args(lshkm_ctx ctx, const AssignRequest& q, const FusedShape& sh, const FusedWorkspace& w) {
    FusedArgs a{};
    a.X = q.X.f64 ? nullptr : q.X.f(); a.X64 = q.X.f64 ? q.X.d() : nullptr;
    a.N = q.N; a.d = q.d; a.K = q.K;
    a.xvec = sh.rows == 1 ? (a.d % 4 == 0 && ((uintptr_t)a.X & 15) == 0) : (a.d % 2 == 0 && ((uintptr_t)a.X64 & 15) == 0);
    a.Ch = w.Ch; a.Cl = w.Cl; a.cnh = w.cnh; a.cbound = w.cbound; a.Kpad = sh.Kpad();
    a.C64 = w.C64p ? w.C64p : q.C; a.Cd = q.C;
    a.C32 = w.C32; a.rn32 = w.rn32; a.fast_dist = sh.fast ? 1 : 0;
    a.assign = q.assign; a.dist = q.dist;
    a.stats = ctx->stats.as<unsigned long long>();
    a.nb = 1;
    if (q.lsh) {
        const ProjTable& pj = q.lsh->proj;
        a.Vh = pj.vh_d.as<_Float16>(); a.Vl = pj.vl_d.as<_Float16>(); a.PT = pj.PT_d.as<double>();
        a.tv = pj.t_d.as<float>(); a.pnorm = pj.pn_d.as<double>(); a.v1 = pj.v1_d.as<double>();
        a.rv = pj.r_d.as<int32_t>(); a.w = pj.w; a.L = pj.L; a.k = pj.k; a.LK = pj.LK; a.LKpad = pj.LKpad;
        a.nb = q.lsh->nb;
    }
    a.bdiv = make_bucket_div(a.nb);
    if (sh.cosine) { a.nbv = w.nbv; a.xn2 = w.xn2; }
    a.cfix = w.cfix; a.cfix_counts = w.seg3; a.cfix_count = w.cfix ? w.cnt + CNT_CFIX : nullptr;
    a.pass_first = 1; a.pass_last = 1;
    return a;
}

// The LSH outputs and the hash fix-up list of the pass that hashes (cosine
// passes list their declined hashes there without hashing too).
void hash_outputs(FusedArgs& a, const AssignRequest& q, const FusedShape& sh, const FusedWorkspace& w) {
    a.hfix = w.hfix; a.hfix_count = w.hfix ? w.cnt + CNT_HFIX : nullptr;
    if (!q.lsh) return;
    a.phi = q.phi; a.bucket = q.bucket;
    a.tuples = sh.cosine ? nullptr : q.tuples ? q.tuples : w.tuples;
}

// One of the call's lists: a segment per block of the plan's grid
template <typename T>
DevList<T> segmented(T* p, unsigned long long* count, int32_t* counts, const AssignRequest& q, const FusedPlan& plan) {
    DevList<T> l;
    l.p = p; l.count = count; l.bound = q.N; l.counts = counts;
    l.seg_rows = plan.seg_rows; l.nseg = plan.nblk;
    return l;
}

// The hi-only passes over all rows; the rows they cannot certify go to list1.
int fused_hi_passes(hipStream_t s, const FusedArgs& hi, const FusedPlan& p) {
    const bool gather_on = !test_switch("LSHKM_GATHER", "0");
    int rc;
    if (p.rows != 0) {
        // general rows: one pass (Kpad <= 512)
        HiForm h;
        h.metric = p.cos; h.rows = p.rows;
        h.fast = !p.cos && hi.fast_dist;
        h.gath = !p.cos && !h.fast && p.rows == 1 && hi.Kpad <= FH_GATH_KMAX && gather_on;
        return launch_fused_hi_pass(s, p.nblk, h, hi);
    }
    // 512 < K <= 1024, euclidean, LSHKM_HI_TWO_IMAGE=1: one two-image launch
    // instead of two passes with carried state. Measured at C5 (N = 10M,
    // K = 1024): 5.09 ms vs 1.83 + 2.51 ms, HBM 8.9 GB vs 13.8 GB per call --
    // the block-wide image swaps line the waves up and cost the MFMA/VALU
    // overlap between them, more than the second read of X costs; opt-in.
    if (!p.cos && p.np_hi == 2 && test_switch("LSHKM_HI_TWO_IMAGE", "1")) {
        HiForm h;
        h.hash = p.hash; h.two_image = true;
        return launch_fused_hi_pass(s, p.nblk, h, hi);
    }
    for (int i = 0; i < p.np_hi; i++) {
        const int c0 = i * FH_KMAX;
        FusedArgs a = hi;
        a.Ch = hi.Ch + (size_t)c0 * FU_D; a.cnh = hi.cnh + c0;
        a.Kpad = std::min(FH_KMAX, hi.Kpad - c0);
        a.t0 = c0 / 32; a.pass_first = i == 0; a.pass_last = i == p.np_hi - 1;
        HiForm h;
        h.hash = p.hash && i == 0; h.mp = p.np_hi > 1; h.metric = p.cos;
        if (!p.cos && !h.mp) {
            // K <= 256: the certified f32 winner distance compiled in, else the
            // winner rows by the LDS-DMA gather (LSHKM_GATHER=0: register loads)
            const bool small = a.Kpad <= FH_GATH_KMAX && gather_on;
            h.fast = small && a.fast_dist;
            h.gath = small && !a.fast_dist;
            // the FAST form fetches its rows one tile ahead (LSHKM_ROW_PREFETCH=0: at the tile's top)
            h.rowpf = h.fast && !test_switch("LSHKM_ROW_PREFETCH", "0");
        } else if (!p.cos) {
            h.fast = !h.hash && a.fast_dist && a.pass_last;
        }
        if ((rc = launch_fused_hi_pass(s, p.nblk, h, a))) return rc;
    }
    return 0;
}

// The 3-product refinement of the rows in list1, FP_KMAX centroids per pass;
// what it cannot certify goes to list2 for the listed exact pass.
int fused_refine_passes(hipStream_t s, const FusedArgs& rf, const FusedPlan& p) {
    for (int i = 0; i < p.np_refine; i++) {
        const int c0 = i * FP_KMAX;
        FusedArgs r = rf;
        r.Ch = rf.Ch + (size_t)c0 * FU_D; r.Cl = rf.Cl + (size_t)c0 * FU_D; r.cnh = rf.cnh + c0;
        r.Kpad = std::min(FP_KMAX, rf.Kpad - c0);
        r.t0 = c0 / 32; r.pass_first = i == 0; r.pass_last = i == p.np_refine - 1;
        const int rc = launch_fused_refine_pass(s, (unsigned)p.nblk, p.cos, p.np_refine > 1, p.rows, r);
        if (rc) return rc;
    }
    return 0;
}

// The side stream between its fork and the main stream's wait on its join
// event. The hash fix-up there writes only tuples / phi / bucket; whatever way
// fused_assign returns after the fork, the fix-up is ordered against later
// work on the main stream: by join(), or by draining the side stream here.
struct SideFork {
    lshkm_ctx c;
    bool open = false;
    int fork() {
        if (hipEventRecord(c->fork_ev, c->stream) != hipSuccess ||
            hipStreamWaitEvent(c->side_stream, c->fork_ev, 0) != hipSuccess)
            return kstatus("fused_assign (fork)");
        open = true;
        return 0;
    }
    // the side stream's work is all enqueued: its timing event, its join event
    int end_side() {
        if (c->timing) {
            if (hipEventRecord(c->tev[2], c->side_stream) != hipSuccess) return kstatus("fused_assign (timing)");
            c->tev_side = true;      // only a call that recorded tev[2] extends the timed pass
        }
        if (hipEventRecord(c->join_ev, c->side_stream) != hipSuccess) return kstatus("fused_assign (join)");
        return 0;
    }
    int join() {
        if (!open) return 0;
        if (hipStreamWaitEvent(c->stream, c->join_ev, 0) != hipSuccess) return kstatus("fused_assign (join)");
        open = false;
        return 0;
    }
    ~SideFork() { if (open) (void)hipStreamSynchronize(c->side_stream); }
};

#ifdef LSHKM_PHASE_TIMING
// Per-phase wave cycles of the passes between its construction and its end,
// printed there.
struct PhaseReport {
    hipStream_t s;
    unsigned long long* d = nullptr;
    explicit PhaseReport(hipStream_t s_) : s(s_) {
        static unsigned long long* prof_d = nullptr;
        if (!prof_d) (void)hipMalloc(&prof_d, 64);
        (void)hipMemsetAsync(prof_d, 0, 64, s);
        d = prof_d;
    }
    ~PhaseReport() {
        unsigned long long v[6];
        (void)hipMemcpyAsync(v, d, 48, hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        // hi-only form: [0] load + split + hash, [1] centroid tiles, [2] certificate + chain + stores
        // (the refinement's fused_persistent_kernel adds its own phases 0-4 over its few rows)
        fprintf(stderr, "PHASES %llu %llu %llu %llu %llu\n", v[0], v[1], v[2], v[3], v[4]);
    }
};
#endif

}  // namespace

int fused_assign(lshkm_ctx ctx, const AssignRequest& q) {
    hipStream_t s = ctx->stream;
    // what the previous call's epilogue left zeroed; the record is dropped until
    // this call's own epilogue is enqueued, so no error return leaves one
    const lshkm_ctx_s::WsClean was_clean = ctx->ws_clean;
    ctx->ws_dirty();
    const bool cosine = q.metric != LSHKM_METRIC_EUCLIDEAN;
    const ProjTable* pj = q.lsh ? &q.lsh->proj : nullptr;
    const FusedRoute route = fused_route(cosine, q.X.f64, q.d, q.K, pj != nullptr, pj ? pj->k : 0, pj ? pj->LK : 0,
                                         test_switch("LSHKM_FUSED_FORM", "chunked"));
    if (route.form == FusedForm::none || (pj && (q.lsh->metric != q.metric || !pj->mfma_ok))) {
        set_error("fused_assign: no fused form runs this shape (fused_route, fused_layout.h)");
        return LSHKM_ERR_ARG;
    }
    FusedShape sh;
    sh.N = q.N; sh.d = q.d; sh.K = q.K; sh.cosine = cosine; sh.rows = route.rows;
    sh.hash = pj != nullptr; sh.LK = pj ? pj->LK : 0;
    // euclidean winner distances: the certified f32 form (the context's default
    // mode) or the reference-order fp64 chain (LSHKM_DIST_EXACT, force_exact)
    sh.fast = !cosine && sh.rows != 2 && !q.force_exact && ctx->dist_mode == LSHKM_DIST_CERTIFIED;
    // the f32 image also serves the K <= 256 gather when every centroid value
    // is an f32 (dataset rows: the first Lloyd iteration), exact as doubles
    // (test switch LSHKM_GATHER32=0: the fp64 winner rows always)
    sh.image32 = sh.fast || (!cosine && sh.rows != 2 && sh.Kpad() <= 256 && !test_switch("LSHKM_GATHER32", "0"));
    sh.own_tuples = sh.hash && !cosine && !q.tuples;
    const bool pwfix = sh.pwfix();
    int rc;
    FusedWorkspace w;
    if ((rc = fused_workspace(ctx, sh, w))) return rc;
    // the counters and the prep's bound words: zero as the last call's epilogue
    // left them, or cleared here (a first call, new allocations, another user since)
    const bool clean = was_clean.cnt == w.cnt && was_clean.cnt_cap == ctx->ws_counter.cap && was_clean.cb == w.cbound &&
                       was_clean.cb_cap == ctx->ws_cconst.cap;
    if (!clean) {
        LSHKM_HIP(hipMemsetAsync(w.cnt, 0, FUSED_COUNTER_CLEAR, s));
        LSHKM_HIP(hipMemsetAsync(w.cbound, 0, FUSED_CBOUND_BYTES, s));
    }
    // the timed fused pass starts before the centroid prep
    if (ctx->timing) LSHKM_HIP(hipEventRecord(ctx->tev[0], s));
    ctx->tev_side = false;
    if ((rc = launch_fused_prep(s, q.C, q.K, q.d, cosine ? 1 : 0, w))) return rc;
    // the listed pass's centroid prep ahead of the passes: it then starts as
    // soon as the refinement ends
    // (not where the refinement settles its leftover rows itself: no listed pass)
    const bool pair_pass = q.N > 0 && route.form != FusedForm::chunked && sh.pairs() && !test_switch("LSHKM_PAIR_PASS", "0");
    const bool settle = pair_pass && !test_switch("LSHKM_SETTLE", "0");
    const bool xprep = !settle && exact_is_pruned(exact_form(q));
    if (xprep && (rc = exact_listed_prep(ctx, q))) return rc;
    if (w.xn2 && (rc = launch_row_sumsq(s, q.X.d(), q.N, q.d, w.xn2))) return rc;

    const FusedArgs common = fused_common_args(ctx, q, sh, w);
    // the rows left for the listed exact pass: flat in list1 (the chunked form;
    // N = 0), else the refinement's segments in list2
    RowList exact_rows;
    exact_rows.p = w.list1; exact_rows.count = w.cnt + CNT_AMBIG; exact_rows.bound = q.N;
    RecList dist_fix[2];      // winners listed for their distance alone
    int ndist_fix = 0;
    RecList pair_rows;        // uncertified rows with both candidates named (bound 0: none)
    SideFork side{ctx};
    if (q.N > 0 && route.form == FusedForm::chunked) {
        FusedArgs a = common;
        hash_outputs(a, q, sh, w);
        a.ambig = w.list1; a.ambig_count = w.cnt + CNT_AMBIG;
        if ((rc = launch_fused_chunked(s, sh.hash, a))) return rc;
    } else if (q.N > 0) {
        FusedPlan p;
        p.hash = sh.hash; p.cos = cosine; p.rows = sh.rows;
        int ncu = 0;
        if (device_cu_count(&ncu)) return LSHKM_ERR_HIP;
        p.nblk = fused_grid(q.N, ncu);
        p.seg_rows = fused_seg_rows(q.N, p.nblk);
        if (p.nblk > FUSED_MAX_SEGS) {       // (then nblk * seg_rows <= list_cap: fused_layout.h)
            set_error("fused_assign: more blocks than list segments");
            return LSHKM_ERR_ARG;
        }
        p.np_hi = (sh.Kpad() + FH_KMAX - 1) / FH_KMAX;
        p.np_refine = (sh.Kpad() + FP_KMAX - 1) / FP_KMAX;
        const RowList l1 = segmented(w.list1, w.cnt + CNT_REFINED, w.seg1, q, p);
        const RecList lh = segmented(w.hfix, w.cnt + CNT_HFIX, w.seg1, q, p);
        const RowList l2 = segmented(w.list2, w.cnt + CNT_AMBIG, w.seg2, q, p);
        FusedArgs seg = common;
        seg.seg_rows = p.seg_rows; seg.part = w.part;
#ifdef LSHKM_PHASE_TIMING
        PhaseReport report(s);
        seg.prof = report.d;
#endif
        FusedArgs hi = seg;
        hash_outputs(hi, q, sh, w);
        hi.ambig = l1.p; hi.ambig_count = l1.count; hi.seg_counts = l1.counts;
        if ((rc = fused_hi_passes(s, hi, p))) return rc;
        // the hash fix-up touches only tuples / phi / bucket of its listed
        // rows: on the side stream, beside the refinement (euclidean: and the
        // listed exact pass), when the context has one
        if (sh.hash) {
            const bool forked = ctx->side_init() == 0;
            if (forked && (rc = side.fork())) return rc;
            launch_hash_fixup(forked ? ctx->side_stream : s, lh, cosine, hi);
            if (forked && (rc = side.end_side())) return rc;
        }
        FusedArgs rf = seg;
        rf.list_in = l1.p; rf.list_counts = l1.counts; rf.list_seg_rows = l1.seg_rows;
        rf.ambig = l2.p; rf.ambig_count = l2.count; rf.seg_counts = l2.counts;
        // its declined cosine distances go to hfix2 (counts beside list2's)
        rf.hfix = cosine ? w.hfix2 : hi.hfix; rf.hfix_count = cosine ? w.cnt + CNT_CFIX : hi.hfix_count;
        // euclidean, one refinement pass: the rows it names both candidates of go
        // to the pair list (counts beside list2's), which each block decides itself
        // before it ends; LSHKM_PAIR_PASS=0: all to list2
        // and with them every other uncertified row is settled by the wave that
        // meets it (counted in list2's slots, not listed); LSHKM_SETTLE=0: to list2
        if (pair_pass) {
            pair_rows = segmented(w.pairs, w.cnt + CNT_PAIR, w.seg2, q, p);
            rf.pairs = pair_rows.p; rf.pair_count = pair_rows.count;
            rf.settle = settle ? 1 : 0;
        }
        if ((rc = fused_refine_passes(s, rf, p))) return rc;
        if (cosine && (rc = side.join())) return rc;
        if ((rc = kstatus("fused_hi_kernel"))) return rc;
        // (with settle, l2's counts -- CNT_AMBIG and the segments' slot 0 -- count rows
        // the refinement decided itself and list2 does not hold: no listed pass on them)
        exact_rows = l2;        if (cosine || pwfix) dist_fix[ndist_fix++] = segmented(w.cfix, w.cnt + CNT_CFIX, w.seg3, q, p);
        if (cosine) dist_fix[ndist_fix++] = segmented(w.hfix2, w.cnt + CNT_CFIX, w.seg2, q, p);
    }
    if (ctx->timing) LSHKM_HIP(hipEventRecord(ctx->tev[1], s));
    if (!settle &&
        (rc = exact_listed(ctx, q, exact_rows, !sh.fast, xprep, cosine ? w.xn2 : nullptr, cosine ? w.nbv : nullptr)))
        return rc;
    // The call's epilogue, one kernel: its counters into the context's, the
    // workspace words zeroed for the next call, the centroid override. It reads
    // and writes nothing the hash fix-up touches, so it runs beside it, before
    // the join; a call with distance fix-up lists joins first and ends with it.
    const bool dist_lists = cosine || pwfix;
    if (dist_lists) {
        if ((rc = side.join())) return rc;
        if ((rc = launch_cos_fix_seg(s, q, ndist_fix, dist_fix, cosine ? w.xn2 : nullptr, cosine ? w.nbv : nullptr)))
            return rc;
    }
    {
        int di[6], n = 0;
        const unsigned long long* sp[6];
        di[n] = STAT_REFINED; sp[n++] = w.cnt + CNT_REFINED;
        if (sh.hash) { di[n] = STAT_HASH_FIX; sp[n++] = w.cnt + CNT_HFIX; }
        di[n] = STAT_ASSIGN_AMBIG; sp[n++] = w.cnt + CNT_AMBIG;
        // pair rows are uncertified rows too (atomic adds: one destination twice is fine)
        if (pair_rows.bound > 0) {
            di[n] = STAT_ASSIGN_AMBIG; sp[n++] = w.cnt + CNT_PAIR;
            di[n] = STAT_PAIR_ROWS; sp[n++] = w.cnt + CNT_PAIR;
        }
        if (dist_lists) { di[n] = cosine ? STAT_COS_FIX : STAT_POW_FIX; sp[n++] = w.cnt + CNT_CFIX; }
        if ((rc = launch_fused_epilogue(s, ctx->stats.as<unsigned long long>(), n, di, sp, w.cnt,
                                        (int)(FUSED_COUNTER_CLEAR / 8), reinterpret_cast<unsigned int*>(w.cbound),
                                        (int)(FUSED_CBOUND_BYTES / 4), q.src_dev, q.K, q.N, q.assign, q.dist)))
            return rc;
    }
    ctx->ws_clean.cnt = w.cnt; ctx->ws_clean.cnt_cap = ctx->ws_counter.cap;
    ctx->ws_clean.cb = w.cbound; ctx->ws_clean.cb_cap = ctx->ws_cconst.cap;
    if ((rc = side.join())) { ctx->ws_dirty(); return rc; }
    return 0;
}

}  // namespace lshkm
