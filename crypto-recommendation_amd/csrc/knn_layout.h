// knn_layout.h — the one statement of lshkm_knn's routing rule and of its
// workspace: which calls the MFMA screen takes, the kept
// capacity, the row groups and segments and the state buffer's regions. The
// f32 images are nearest_layout.h's (nearest_image). Plain host arithmetic: no
// HIP.
#pragma once
#include "nearest_layout.h"

namespace lshkm {

constexpr int KNN_KMAX = 64;                   // = LSHKM_KNN_KMAX: a result slot per lane of the settling wave

// ---- the kept capacity per query: the k rows that set the threshold are
// always kept; the slack takes the rows the threshold lets in beside them
// (groups that hold two of the k nearest, intervals that overlap the cut).
// small: the test build's LSHKM_KNN_CAP=small.
inline int knn_cap(int k, bool small) { return small ? k : 2 * k + 32; }
constexpr int KNN_CAP_MAX = 2 * KNN_KMAX + 32;

// ---- row groups: disjoint contiguous ranges of grp_rows = 32 * 2^j rows (one
// 32-row MFMA tile at the least), as fine as the key array's bounds allow: at
// most KNN_GROUPS_MAX groups (the select wave holds a query's keys in
// registers) and at most KNN_KEYS_MAX (query, group) keys in all (128 MiB).
// The threshold of a query is the k-th smallest of its groups' minima, so the
// screen needs at least k groups.
constexpr int KNN_GRP_MIN = 32;
constexpr int KNN_GROUPS_MAX = 1024;
constexpr int64_t KNN_KEYS_MAX = (int64_t)1 << 25;

// ---- row segments (a block's share of the rows): whole groups and whole LDS
// stages, sized as nearest_plan sizes its own.
struct KnnPlan {
    int cap;
    int groups;              // 0: the key array's bound leaves no group (the scan's)
    int grp_shift;           // grp_rows = 1 << grp_shift
    int64_t grp_rows;
    int segs;
    int64_t seg_rows;        // a multiple of grp_rows and of NEAREST_STAGE
    int64_t tiles;           // query tiles of NEAREST_COLS
};
// small_seg: the test build's LSHKM_KNN_SEG=small (groups and segments of one
// LDS stage where the bounds allow).
inline KnnPlan knn_plan(int64_t N, int64_t nq, int k, int ncu, bool small_cap, bool small_seg) {
    KnnPlan p;
    p.cap = knn_cap(k, small_cap);
    p.tiles = std::max<int64_t>(1, (nq + NEAREST_COLS - 1) / NEAREST_COLS);
    const int64_t gmax = std::min<int64_t>(KNN_GROUPS_MAX, KNN_KEYS_MAX / std::max<int64_t>(nq, 1));
    p.grp_shift = small_seg ? 6 : 5;
    while (((N + ((int64_t)1 << p.grp_shift) - 1) >> p.grp_shift) > std::max<int64_t>(gmax, 1)) p.grp_shift++;
    p.grp_rows = (int64_t)1 << p.grp_shift;
    p.groups = gmax < 1 ? 0 : (int)((N + p.grp_rows - 1) / p.grp_rows);
    const int64_t unit = std::max<int64_t>(p.grp_rows, NEAREST_STAGE);
    const int64_t seg_min = small_seg ? unit : std::max<int64_t>(NEAREST_SEG_MIN, unit);
    const int64_t by_rows = small_seg ? std::max<int64_t>(1, (N + seg_min - 1) / seg_min) : std::max<int64_t>(1, N / seg_min);
    const int64_t by_fill =
        small_seg ? by_rows : std::max<int64_t>(1, (NEAREST_FILL * (int64_t)std::max(ncu, 1) + p.tiles - 1) / p.tiles);
    p.segs = (int)std::min<int64_t>(NEAREST_SEG_MAX, std::min(by_rows, by_fill));
    const int64_t per = (N + p.segs - 1) / p.segs;
    p.seg_rows = std::max<int64_t>(unit, (per + unit - 1) / unit * unit);
    p.segs = (int)std::max<int64_t>(1, (N + p.seg_rows - 1) / p.seg_rows);
    return p;
}

// ---- the routing rule. screen: rows of at most NEAREST_DMAX dims, at least k
// groups, at most NEAREST_POISON_MAX poison rows and at least k real rows (the
// last two known only after the prep: knn_route_after_prep); scan: everything
// else, and every query the screen hands back (a poison query, fewer than k
// groups with a real row, a kept-list overflow).
enum class KnnRoute { screen, scan };
inline KnnRoute knn_route(int d, int k, int groups, bool force_scan) {
    return (force_scan || d > NEAREST_DMAX || groups < k) ? KnnRoute::scan : KnnRoute::screen;
}
inline KnnRoute knn_route_after_prep(int64_t N, int k, int64_t poison_rows) {
    return (poison_rows > NEAREST_POISON_MAX || N - poison_rows < k) ? KnnRoute::scan : KnnRoute::screen;
}

// ---- the call's state: gkey (uint32 [nq][groups]: the order-preserving key of
// each group's smallest hi; all ones = no real row) | tau (uint32 [nq]: the
// k-th smallest of them; all ones = none) | cnt (int32 [nq]: rows with lo <=
// tau) | krow (int32 [nq][cap]) | scan (int32 [nq]: the queries handed to the
// exact scan) | pois (int32 [NEAREST_POISON_MAX]) | counts (uint32 [4]: as
// nearest_layout.h's NEAREST_N_*)
struct KnnState {
    size_t gkey, tau, cnt, krow, scan, pois, counts, bytes;
};
inline KnnState knn_state(int64_t nq, int groups, int cap) {
    const size_t m = (size_t)std::max<int64_t>(nq, 1);
    KnnState l;
    l.gkey = 0;
    l.tau = nearest_round256(4 * m * (size_t)std::max(groups, 1));
    l.cnt = l.tau + nearest_round256(4 * m);
    l.krow = l.cnt + nearest_round256(4 * m);
    l.scan = l.krow + nearest_round256(4 * m * (size_t)cap);
    l.pois = l.scan + nearest_round256(4 * m);
    l.counts = l.pois + nearest_round256(4 * (size_t)NEAREST_POISON_MAX);
    l.bytes = l.counts + 256;
    return l;
}

}  // namespace lshkm
