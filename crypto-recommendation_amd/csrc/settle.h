// settle.h — the candidate sets of the rows the fused refinement settles itself
// (fused_refine.hip): where a score's bit sits in a lane's mask, which centroid
// it names, the row's set in centroid order from its two lanes' masks, and the
// k-th candidate of a set (the listed pruned pass selects the same way,
// exact_pass.hip). Plain integer arithmetic, host and device
// (tests/settle_mask_check.cpp runs it over every position).
//
// A lane of half h holds, of its row, score i (0..15) of every 32-centroid tile
// t (0..7): centroid 32 t + 8 (i / 4) + 4 h + i % 4 (the MFMA's D layout,
// tile_scores). Its mask is 128 bits, bit 16 t + i: tiles 0-3 in lo, 4-7 in hi.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ST_HD __host__ __device__ inline
#else
#define ST_HD inline
#endif

namespace lshkm {

constexpr int ST_TILES = 8;                  // 32-centroid tiles a mask covers (Kpad <= 256)
constexpr int ST_CHUNKS = ST_TILES / 2;      // 64-centroid chunks of a row's set

struct LaneMask {
    unsigned long long lo, hi;
};

// the centroid behind score i of tile t in lane half h
ST_HD int settle_centroid(int h, int t, int i) { return 32 * t + 8 * (i >> 2) + 4 * h + (i & 3); }

// one tile's 16 flags (bit i: score i is a candidate) into the lane's mask
ST_HD void settle_mark(LaneMask& m, int t, uint32_t bits16) {
    const unsigned long long b = (unsigned long long)(bits16 & 0xFFFFu) << (16 * (t & 3));
    if (t < 4) m.lo |= b; else m.hi |= b;
}

// Two tiles' flags (32 bits) spread to their 64 centroids' places for half 0:
// nibble g of tile t' moves to bit 32 t' + 8 g; half 1's sit 4 higher.
ST_HD unsigned long long settle_spread(uint32_t two_tiles) {
    unsigned long long x = two_tiles;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    return x;
}

// The row's candidate set in centroid order (bit c % 64 of cm[c / 64]) from
// its lower (h = 0) and upper (h = 1) lane's masks, without the centroids from
// K on (padding rows of the image); returns the number of candidates.
ST_HD int settle_set(const LaneMask& m0, const LaneMask& m1, int K, unsigned long long (&cm)[ST_CHUNKS]) {
    cm[0] = settle_spread((uint32_t)m0.lo) | (settle_spread((uint32_t)m1.lo) << 4);
    cm[1] = settle_spread((uint32_t)(m0.lo >> 32)) | (settle_spread((uint32_t)(m1.lo >> 32)) << 4);
    cm[2] = settle_spread((uint32_t)m0.hi) | (settle_spread((uint32_t)m1.hi) << 4);
    cm[3] = settle_spread((uint32_t)(m0.hi >> 32)) | (settle_spread((uint32_t)(m1.hi >> 32)) << 4);
    int n = 0;
    for (int i = 0; i < ST_CHUNKS; i++) {
        const int left = K - 64 * i;
        if (left < 64) cm[i] &= left <= 0 ? 0ull : (1ull << left) - 1ull;
        n += __builtin_popcountll(cm[i]);
    }
    return n;
}

// The k-th candidate of a set (increasing c), or -1 past the last.
template <int NCH>
ST_HD int kth_candidate(const unsigned long long (&cm)[NCH], int k) {
    int c = -1, seen = 0;
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        const int n = __builtin_popcountll(cm[i]);
        if (c < 0 && k >= seen && k < seen + n) {
            unsigned long long m = cm[i];
            for (int t = k - seen; t > 0; t--) m &= m - 1;
            c = 64 * i + __builtin_ctzll(m);
        }
        seen += n;
    }
    return c;
}

}  // namespace lshkm
