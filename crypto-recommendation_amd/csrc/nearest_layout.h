// nearest_layout.h — the one statement of lshkm_min_vector_dist's routing rule
// and of its workspace: which calls the MFMA screen takes, the kept capacity,
// the row segments and every buffer's regions. Plain host arithmetic: no HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace lshkm {

// ---- the routing rule. screen: rows of at most NEAREST_DMAX dims (the MFMA's
// B operand in registers) and at most NEAREST_POISON_MAX poison rows (known
// only after the prep: nearest_route_after_prep); scan: everything else, and
// every query the screen hands back (a poison query, a kept-list overflow).
constexpr int NEAREST_DMAX = 128;
constexpr int NEAREST_STAGE = 64;        // rows staged in LDS per step
constexpr int NEAREST_COLS = 128;        // queries per block (32 per wave)
constexpr int NEAREST_CAP = 32;          // kept rows per query
constexpr int NEAREST_CAP_MIN = 1;       // the row that sets the threshold is always kept
constexpr int NEAREST_POISON_MAX = 16;   // poison rows the settle takes on for every query
enum class NearestRoute { screen, scan };

inline NearestRoute nearest_route(int d, bool force_scan) {
    return (force_scan || d > NEAREST_DMAX) ? NearestRoute::scan : NearestRoute::screen;
}
inline NearestRoute nearest_route_after_prep(int64_t poison_rows) {
    return poison_rows > NEAREST_POISON_MAX ? NearestRoute::scan : NearestRoute::screen;
}
// small: the test build's LSHKM_NEAREST_CAP=small.
inline int nearest_cap(bool small) { return small ? NEAREST_CAP_MIN : NEAREST_CAP; }
// Padded dims of the f32 image (the screen kernel's two instantiations).
inline int nearest_dp(int d) { return d <= 32 ? 32 : 128; }

// ---- row segments: as many as give NEAREST_FILL (query tile, segment) blocks
// per CU, each a multiple of NEAREST_STAGE rows and at least seg_min of them
// (NEAREST_SEG_MIN, or one stage with the test build's LSHKM_NEAREST_SEG=small),
// at most NEAREST_SEG_MAX segments.
constexpr int64_t NEAREST_SEG_MIN = 1024;
constexpr int NEAREST_SEG_MAX = 4096;
constexpr int NEAREST_FILL = 8;
struct NearestPlan {
    int cap, segs;
    int64_t seg_rows;        // rows per segment (a multiple of NEAREST_STAGE)
    int64_t tiles;           // query tiles of NEAREST_COLS
};
inline NearestPlan nearest_plan(int64_t N, int64_t nq, int ncu, bool small_cap, bool small_seg) {
    NearestPlan p;
    p.cap = nearest_cap(small_cap);
    p.tiles = std::max<int64_t>(1, (nq + NEAREST_COLS - 1) / NEAREST_COLS);
    const int64_t seg_min = small_seg ? NEAREST_STAGE : NEAREST_SEG_MIN;
    const int64_t by_rows = small_seg ? std::max<int64_t>(1, (N + seg_min - 1) / seg_min) : std::max<int64_t>(1, N / seg_min);
    const int64_t by_fill =
        small_seg ? by_rows : std::max<int64_t>(1, (NEAREST_FILL * (int64_t)std::max(ncu, 1) + p.tiles - 1) / p.tiles);
    p.segs = (int)std::min<int64_t>(NEAREST_SEG_MAX, std::min(by_rows, by_fill));
    const int64_t per = (N + p.segs - 1) / p.segs;
    p.seg_rows = std::max<int64_t>(NEAREST_STAGE, (per + NEAREST_STAGE - 1) / NEAREST_STAGE * NEAREST_STAGE);
    p.segs = (int)std::max<int64_t>(1, (N + p.seg_rows - 1) / p.seg_rows);
    return p;
}

inline size_t nearest_round256(size_t b) { return (b + 255) / 256 * 256; }

// ---- the f32 image of one side (the rows, or the queries): x^ [n][dp] f32 |
// a (f32 [n]: |x^|^2 euclidean, 1 / |x^| cosine; negative = poison) | rel (f32
// [n]: the conversion term of the bound) | xa (double [n]: the reference's sum
// of squares, cosine on fp64 values). dp = 0 (the lists form): xa alone.
struct NearestImage {
    size_t xh, a, rel, xa, bytes;
};
inline NearestImage nearest_image(int64_t n, int dp) {
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    NearestImage l;
    l.xh = 0;
    l.a = nearest_round256(4 * m * dp);
    l.rel = l.a + nearest_round256(4 * m);
    l.xa = l.rel + nearest_round256(4 * m);
    l.bytes = l.xa + nearest_round256(8 * m);
    return l;
}

// ---- the call's state: minkey (uint32 [nq]: the order-preserving key of the
// smallest hi) | cnt (int32 [nq]: rows with lo <= it) | krow (int32 [nq][cap])
// | scan (int32 [nq]: the queries handed to the exact scan) | pois (int32
// [NEAREST_POISON_MAX]) | counts (uint32 [4]: poison rows, scan queries, list
// errors)
struct NearestState {
    size_t minkey, cnt, krow, scan, pois, counts, bytes;
};
inline NearestState nearest_state(int64_t nq, int cap) {
    const size_t m = (size_t)std::max<int64_t>(nq, 1);
    NearestState l;
    l.minkey = 0;
    l.cnt = nearest_round256(4 * m);
    l.krow = l.cnt + nearest_round256(4 * m);
    l.scan = l.krow + nearest_round256(4 * m * (size_t)cap);
    l.pois = l.scan + nearest_round256(4 * m);
    l.counts = l.pois + nearest_round256(4 * (size_t)NEAREST_POISON_MAX);
    l.bytes = l.counts + 256;
    return l;
}
constexpr int NEAREST_N_POISON = 0, NEAREST_N_SCAN = 1, NEAREST_N_BADIDX = 2;

}  // namespace lshkm
