// Host check of csrc/exact_layout.h (tests/test_exact_layout_cpu.py): the exact
// pass's routing rule against the predicates it replaced and at its edges, the
// workspace against the extent each form's kernels touch, its regions, and the
// grids.
#include <cstdio>

#include "../crypto-recommendation_amd/csrc/exact_layout.h"

using namespace lshkm;

static long bad = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) { bad++; if (bad < 20) std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

// The rule as the host code spelled it before exact_route: exact_pruned(), the
// condition of exact_listed() (a flat list never had d > 256 pruned or batched)
// and the launcher's `wide`.
static ExactForm old_route(bool cosine, bool f64, int d, int K, bool full) {
    const bool prune = K <= 1024 && d <= 256 && !full && (!cosine || !f64);
    if (prune) return (K + 63) / 64 * 64 > 256 ? ExactForm::pruned_wide : ExactForm::pruned;
    if (cosine || d > 256) return ExactForm::every;
    return ExactForm::batch;
}

// Bytes past the workspace's start that a form's kernels read or write.
static size_t touched(ExactForm f, int d, int K) {
    if (f == ExactForm::batch) {
        // transpose_centroids_kernel: CT[j * Kp + c], j < d, c < Kp; the pass reads
        // column c0 + lane + 64 i <= 256 ceil(K / 256) - 1 of rows j < d
        const size_t Kp = (size_t)(K + 255) / 256 * 256;
        return ((size_t)(d - 1) * Kp + Kp) * 8;
    }
    if (f == ExactForm::every) return 0;
    // exact_prep_kernel: CT32[j * Kp + c] (j < d, c < Kp), cconst[c] (c < Kp), two
    // maxima per chunk of 64 centroids (cleared, then atomicMax)
    const size_t Kp = (size_t)(K + 63) / 64 * 64;
    return 4 * ((size_t)d * Kp + Kp + 2 * (Kp / 64));
}

int main() {
    for (int cosine = 0; cosine < 2; cosine++)
        for (int f64 = 0; f64 < 2; f64++)
            for (int full = 0; full < 2; full++)
                for (int d = 1; d <= 257; d++)
                    for (int K = 1; K <= 1100; K++) {
                        const ExactForm f = exact_route(cosine, f64, d, K, full);
                        CHECK(f == old_route(cosine, f64, d, K, full));
                        const ExactWs w = exact_ws(f, d, K);
                        CHECK(exact_ws_bytes(f, d, K) == w.bytes && w.bytes >= touched(f, d, K));
                        // the regions: in order, disjoint, 4-B aligned (CT: 8)
                        CHECK(w.ct == 0 && w.ct <= w.cconst && w.cconst <= w.chunk && w.chunk <= w.bytes);
                        CHECK(w.cconst % 4 == 0 && w.chunk % 4 == 0 && w.bytes % 4 == 0);
                        if (exact_is_pruned(f)) {
                            CHECK(w.Kpad % 64 == 0 && w.Kpad >= K && w.Kpad - K < 64);
                            CHECK((f == ExactForm::pruned_wide) == (w.Kpad > 256) && w.Kpad <= 64 * 16);
                            CHECK(w.cconst - w.ct >= 4 * (size_t)d * w.Kpad);
                            CHECK(w.chunk - w.cconst >= 4 * (size_t)w.Kpad);
                            CHECK(w.bytes - w.chunk >= 4 * (size_t)2 * (w.Kpad / 64));
                        } else if (f == ExactForm::batch) {
                            CHECK(w.Kpad % 256 == 0 && w.Kpad >= K && w.bytes % 8 == 0);
                        } else {
                            CHECK(w.bytes == 0);
                        }
                    }
    // the edges, where they have always been
    CHECK(exact_route(false, false, 128, 256, false) == ExactForm::pruned);
    CHECK(exact_route(false, false, 128, 257, false) == ExactForm::pruned_wide);
    CHECK(exact_route(false, false, 128, 1024, false) == ExactForm::pruned_wide);
    CHECK(exact_route(false, false, 128, 1025, false) == ExactForm::batch);
    CHECK(exact_route(true, false, 128, 1024, false) == ExactForm::pruned_wide);
    CHECK(exact_route(true, false, 128, 1025, false) == ExactForm::every);
    CHECK(exact_route(false, true, 256, 64, false) == ExactForm::pruned);
    CHECK(exact_route(false, true, 257, 64, false) == ExactForm::every);
    CHECK(exact_route(true, true, 100, 64, false) == ExactForm::every);
    CHECK(exact_route(false, false, 128, 64, true) == ExactForm::batch);
    CHECK(exact_route(true, false, 128, 64, true) == ExactForm::every);
    // d = 1, K = 256: 2080 B touched. The fp64 CT's formula, d * ceil256(K) * 8 =
    // 2048 B, was reserved for every form before and is 32 B short of it.
    CHECK(touched(ExactForm::pruned, 1, 256) == 2080 && exact_ws_bytes(ExactForm::pruned, 1, 256) == 2080);
    CHECK((size_t)1 * 256 * 8 < touched(ExactForm::pruned, 1, 256));

    // the grids, as the launchers computed them
    for (int64_t bound : {(int64_t)1, (int64_t)3, (int64_t)4, (int64_t)33, (int64_t)1037, (int64_t)40000, (int64_t)10000000}) {
        CHECK(exact_blocks(ExactForm::every, 0, bound, true) == std::min<int64_t>((bound + 3) / 4, 256));
        CHECK(exact_blocks(ExactForm::every, 0, bound, false) == std::min<int64_t>((bound + 3) / 4, 2048));
        CHECK(exact_blocks(ExactForm::batch, 0, bound, true) == std::min<int64_t>(((bound + 7) / 8 + 3) / 4, 2048));
        CHECK(exact_blocks(ExactForm::pruned, 0, bound, true) == std::min<int64_t>(((bound + 7) / 8 + 3) / 4, 2048));
        for (int nseg : {0, 1, 256, FUSED_MAX_SEGS})
            CHECK(exact_blocks(ExactForm::pruned_wide, nseg, bound, true) == std::min<int64_t>(((bound + 3) / 4 + 3) / 4, 1024));
        for (int nseg : {1, 256, FUSED_MAX_SEGS}) {
            CHECK(exact_blocks(ExactForm::every, nseg, bound, true) == 2 * nseg);
            CHECK(exact_blocks(ExactForm::batch, nseg, bound, true) == 4 * nseg);
            CHECK(exact_blocks(ExactForm::pruned, nseg, bound, true) == 4 * nseg);
        }
    }
    std::printf("bad=%ld\n", bad);
    return bad ? 1 : 0;
}
