// exact_layout.h — the one statement of the listed exact pass's routing rule,
// of its kernels' shapes and of its workspace (exact_pass.hip; reserved by
// exact_listed, api.cpp). Plain host arithmetic: no HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "fused_layout.h"

namespace lshkm {

// ---- the forms. Every one gives the reference's first minimum over all K
// centroids in its exact order, for the rows of a list:
//   every        a wave per row, lane c takes centroids c, c + 64, ...
//                (any d, K and metric; also the all-rows pass);
//   batch        euclidean: XB_R rows per wave against a transposed fp64 copy
//                of the centroids;
//   pruned       K <= XP_KMAX: every centroid scored in f32 first, the exact
//                order only on the candidates the bound leaves; XP_R rows per
//                wave over 4 chunks of 64 centroids, XP_SPLIT blocks per
//                list segment;
//   pruned_wide  the same over 16 chunks (ceil64(K) > 256): XPW_R rows per
//                wave, the segments' groups dealt in one flat index space.
enum class ExactForm { every, batch, pruned, pruned_wide };

constexpr int XB_DMAX = 256;     // row length the LDS-staged forms hold
constexpr int XP_KMAX = 1024;    // 16 chunks of 64 centroids per lane
constexpr int XE_WAVES = 4, XE_SPLIT = 2;               // every: waves per block, blocks per list segment
constexpr int XB_R = 8, XB_WAVES = 4, XB_SPLIT = 4;     // batch: 16 waves per CU hide the CT-load latency
constexpr int XP_R = 8, XP_WAVES = 4, XP_SPLIT = 4;     // pruned
constexpr int XPW_R = 4;                                // pruned_wide (its waves per block: XP_WAVES)

inline int exact_kpad(int K, int to) { return (K + to - 1) / to * to; }

// full_switch: the test build's LSHKM_EXACT_PASS=full (no pruning). Cosine
// prunes fp32 rows only.
inline ExactForm exact_route(bool cosine, bool f64, int d, int K, bool full_switch) {
    if (K <= XP_KMAX && d <= XB_DMAX && !full_switch && (!cosine || !f64))
        return exact_kpad(K, 64) > 256 ? ExactForm::pruned_wide : ExactForm::pruned;
    return !cosine && d <= XB_DMAX ? ExactForm::batch : ExactForm::every;
}
inline bool exact_is_pruned(ExactForm f) { return f == ExactForm::pruned || f == ExactForm::pruned_wide; }

// ---- the workspace. batch: CT [d][Kpad] doubles, Kpad = ceil256(K) (whole
// 256-centroid passes, no bounds checks). pruned forms, Kpad = ceil64(K): CT32
// [d][Kpad] floats, cconst [Kpad] floats, then {ec, eb} per chunk of 64
// centroids, 2 Kpad / 64 floats. every: none.
struct ExactWs {
    int Kpad = 0;
    size_t ct = 0, cconst = 0, chunk = 0, bytes = 0;     // byte offsets (ct: CT or CT32)
};
inline ExactWs exact_ws(ExactForm f, int d, int K) {
    ExactWs w;
    if (f == ExactForm::batch) {
        w.Kpad = exact_kpad(K, 256);
        w.cconst = w.chunk = w.bytes = (size_t)d * w.Kpad * 8;
    } else if (exact_is_pruned(f)) {
        w.Kpad = exact_kpad(K, 64);
        w.cconst = (size_t)d * w.Kpad * 4;
        w.chunk = w.cconst + (size_t)w.Kpad * 4;
        w.bytes = w.chunk + (size_t)(w.Kpad / 64) * 2 * 4;
    }
    return w;
}
inline size_t exact_ws_bytes(ExactForm f, int d, int K) { return exact_ws(f, d, K).bytes; }

// ---- the grid. A segmented list (nseg > 0, the fused kernels' lists): the
// form's split blocks per segment, except pruned_wide's flat group space; a flat
// list of at most bound rows: a wave per row (every; listed: the list is
// usually ~0.3% of the rows) or per group of R rows.
inline int64_t exact_blocks(ExactForm f, int nseg, int64_t bound, bool listed) {
    const auto per = [&](int R, int waves, int64_t cap) {
        return std::min<int64_t>(((bound + R - 1) / R + waves - 1) / waves, cap);
    };
    switch (f) {
        case ExactForm::every: return nseg > 0 ? (int64_t)nseg * XE_SPLIT : per(1, XE_WAVES, listed ? 256 : 2048);
        case ExactForm::batch: return nseg > 0 ? (int64_t)nseg * XB_SPLIT : per(XB_R, XB_WAVES, 2048);
        case ExactForm::pruned: return nseg > 0 ? (int64_t)nseg * XP_SPLIT : per(XP_R, XP_WAVES, 2048);
        default: return per(XPW_R, XP_WAVES, 1024);
    }
}

}  // namespace lshkm
