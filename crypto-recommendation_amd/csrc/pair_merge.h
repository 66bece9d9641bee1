// pair_merge.h — the refinement's named runner-up: the running top three of a
// lane's scores with the tiles of the first two, and the merge of a row's two
// lane halves. Plain arithmetic, host and device (tests/pair_merge_check.cpp
// runs it against a sort).
//
// Scores are floats compared by value; equal values are legal everywhere (a
// score's low mantissa bits carry its in-tile index, so two tiles can hold the
// same bits). What the state promises, whatever the ties:
//   m1 >= m2 >= m3; (m1, t1) and (m2, t2) are two different scores of the
//   lane, each with the tile it came from; m3 >= every other score of the lane.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PM_HD __host__ __device__ inline
#else
#define PM_HD inline
#endif

namespace lshkm {

struct Top3 {
    float m1, m2, m3;
    int t1, t2;
};

// One more score v of tile t. A new maximum only by strict '>': the first tile
// that reaches the maximum keeps it (tile_epilogue's t1). A score equal to m1
// becomes the runner-up with ITS tile; one equal to m2 falls to m3, which then
// equals m2 -- such a row is never a pair row.
PM_HD void top3_insert(Top3& s, float v, int t) {
    const bool gt1 = v > s.m1, gt2 = v > s.m2;
    s.m3 = gt2 ? s.m2 : (v > s.m3 ? v : s.m3);
    s.t2 = gt1 ? s.t1 : (gt2 ? t : s.t2);
    s.m2 = gt1 ? s.m1 : (gt2 ? v : s.m2);
    s.t1 = gt1 ? t : s.t1;
    s.m1 = gt1 ? v : s.m1;
}

// The two lane halves of one row, each with its best two scores as (value,
// centroid index) and its m3. w is the half the caller took the winner I1 =
// w.i1 from (w.m1 >= l.m1), l the other: the row's runner-up index I2 and M3,
// the bound on every score of the row but the two named. The runner-up is the
// better of w's second and l's first; on a tie between them M3 equals the
// runner-up's score.
struct HalfTop {
    float m1, m2, m3;
    int i1, i2;
};
struct PairMerge {
    int I2;
    float M3;
};
PM_HD PairMerge merge_halves(const HalfTop& w, const HalfTop& l) {
    PairMerge r;
    if (l.m1 > w.m2) {      // l's best is the runner-up: w.m2, l.m2 and below remain
        r.I2 = l.i1;
        r.M3 = w.m2 > l.m2 ? w.m2 : l.m2;
    } else {                // w's second is: l.m1, w.m3 and below remain
        r.I2 = w.i2;
        r.M3 = w.m3 > l.m1 ? w.m3 : l.m1;
    }
    return r;
}

}  // namespace lshkm
