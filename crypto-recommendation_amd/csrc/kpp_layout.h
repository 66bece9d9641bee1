// kpp_layout.h — the one map of the k-means++ workspace of one device or one shard
// (kmeanspp.hip; reserved by api.cpp, sized for callers by lshkm_kpp_shard_ws_bytes)
// and the record a shard's steps leave for the host. Plain host arithmetic: no HIP.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kpp_chain.h"

namespace lshkm {

constexpr int KPP_GROUP = 256;            // rows per pass of a distance block = per approximate sum m^2
constexpr int KPP_DIST_BLOCKS = 4096;     // cap on distance blocks = per-block maxima held
static_assert(KPP_CHUNK == 2 * KPP_GROUP, "two row groups per chunk");

// What a shard's steps leave for the host (lshkm_kpp_shard_*), in the 64-byte
// slot of the max word, right behind it.
struct KppShardOut {
    unsigned long long max_bits;   // dist: the shard's max of minima (0 if none)
    double sum;                    // dist: its approximate sum m^2
    double s_out;                  // chain: the running sum after its rows
    long long pick;                // pick: a local row, or -1
};
static_assert(8 + sizeof(KppShardOut) <= 64, "the max word's 64 bytes hold the shard's outputs");

// Byte offsets of the regions, in this order: mind, the running minima, and
// cum, the stop chunks' prefix sums, [N] f64 each; gsum, sum m^2 per row group
// (an even count); per chunk the approximate start, the record, the exact start
// cs (f64) and the mode (i32, an even count); the max word mx with `out` behind
// it; the per-block maxima; q [N] f64 and the prefix arrays pa, pb [N] i64.
struct KppLayout {
    int64_t nch, ngroups;
    unsigned dgrid;                // blocks of the distance pass
    size_t mind, cum, gsum, cstart, meta, cs, mode, mx, out, bmax, qbuf, pa, pb, bytes;
};
inline KppLayout kpp_layout(int64_t N) {
    KppLayout w;
    w.nch = (N + KPP_CHUNK - 1) / KPP_CHUNK;
    w.ngroups = (N + KPP_GROUP - 1) / KPP_GROUP;
    w.dgrid = (unsigned)(w.ngroups < 1 ? 1 : w.ngroups > KPP_DIST_BLOCKS ? KPP_DIST_BLOCKS : w.ngroups);
    size_t p = 0;
    const auto take = [&p](size_t size, int64_t count) { const size_t at = p; p += size * (size_t)count; return at; };
    w.mind = take(8, N);                            w.cum = take(8, N);
    w.gsum = take(8, (w.ngroups + 1) & ~1ll);       w.cstart = take(8, w.nch);
    w.meta = take(sizeof(KppChunk), w.nch);         w.cs = take(8, w.nch);
    w.mode = take(4, (w.nch + 1) & ~1ll);           w.mx = take(64, 1);
    w.out = w.mx + 8;                               w.bmax = take(8, KPP_DIST_BLOCKS);
    w.qbuf = take(8, N);                            w.pa = take(8, N);
    w.pb = take(8, N);                              w.bytes = p;
    return w;
}

}  // namespace lshkm
