// lshpc_layout.h — the one statement of lshkm_lsh_p_closest's routing rule and
// of its workspaces: which calls the MFMA screen takes, the kept-list capacity,
// the row segments, the user chunks and every buffer's regions. Plain host
// arithmetic: no HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace lshkm {

// ---- the routing rule. screen: a cosine handle whose L bucket IDs of k bits
// pack into one uint32, rows of at most LSHPC_DMAX dims (the MFMA's B operand
// in registers), and a P whose kept-list fits LSHPC_CAP_MAX entries; lists:
// everything else, and every user the screen hands back (poison, overflow,
// tie / NaN): lshkm_lsh_query_f64 -> lshkm_cv_exclude -> lshkm_p_closest on
// those users, gathered.
constexpr int LSHPC_DMAX = 128;
constexpr int LSHPC_CODE_BITS = 32;
constexpr int LSHPC_STAGE = 64;          // pool rows staged in LDS per step: a list grows by at most this between prunes
constexpr int LSHPC_COLS = 128;          // users per block (32 per wave)
constexpr int LSHPC_CAP = 256;           // kept-list entries per (user, segment)
constexpr int LSHPC_CAP_MAX = 512;       // 8 entries per lane of the pruning wave
enum class LshpcRoute { screen, lists };

// The smallest legal capacity: after a prune the P + 1 entries that set the
// threshold stay, and the next step appends up to LSHPC_STAGE more.
inline int lshpc_cap_min(int P) { return P + 1 + LSHPC_STAGE; }
// small: the test build's LSHKM_LSHPC_CAP=small.
inline int lshpc_cap(int P, bool small) {
    if (small) return lshpc_cap_min(P);
    return (int)std::max<int64_t>(LSHPC_CAP, std::min<int64_t>(LSHPC_CAP_MAX, 2 * ((int64_t)P + 1) + LSHPC_STAGE));
}
inline LshpcRoute lshpc_route(bool cosine, int d, int L, int k, int P, bool force_lists) {
    if (force_lists || !cosine || d > LSHPC_DMAX || (int64_t)L * k > LSHPC_CODE_BITS) return LshpcRoute::lists;
    return (int64_t)P + 1 + LSHPC_STAGE <= LSHPC_CAP_MAX ? LshpcRoute::screen : LshpcRoute::lists;
}
// Padded dims of the f32 image (the screen kernel's two instantiations).
inline int lshpc_dp(int d) { return d <= 32 ? 32 : 128; }

inline size_t lshpc_round256(size_t b) { return (b + 255) / 256 * 256; }

// ---- the f32 image of rows (the pool, or the users): x^ [n][dp] f32 | code
// (uint32 [n]) | inv (f32 [n]: 1 / |x^|, negative = poison) | rel (f32 [n]:
// the conversion term of the bound) | xa (double [n]: the reference's sum of
// squares) | bucket (int32 [n][L], the users' only)
struct LshpcImage {
    size_t xh, code, inv, rel, xa, bucket, bytes;
};
inline LshpcImage lshpc_image(int64_t n, int dp, int L_users) {
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    LshpcImage l;
    l.xh = 0;
    l.code = lshpc_round256(4 * m * dp);
    l.inv = l.code + lshpc_round256(4 * m);
    l.rel = l.inv + lshpc_round256(4 * m);
    l.xa = l.rel + lshpc_round256(4 * m);
    l.bucket = l.xa + lshpc_round256(8 * m);
    l.bytes = l.bucket + lshpc_round256(4 * m * (size_t)L_users);
    return l;
}

// ---- one chunk of users. Row segments: as many as give LSHPC_FILL (user tile,
// segment) blocks per CU (two or three are resident: several rounds, so that
// the last one's idle CUs cost little), each a multiple of LSHPC_STAGE rows and
// at least LSHPC_SEG_MIN of them, at most LSHPC_SEG_MAX.
constexpr int64_t LSHPC_SEG_MIN = 1024;
constexpr int LSHPC_SEG_MAX = 64;
constexpr int LSHPC_FILL = 8;
constexpr size_t LSHPC_BUDGET = (size_t)1 << 30;       // the chunk's workspace, bytes
struct LshpcPlan {
    int cap, segs;
    int64_t seg_rows;        // rows per segment (a multiple of LSHPC_STAGE)
    int64_t chunk;           // users per chunk (a multiple of LSHPC_COLS, or nq)
};
// Per user of a chunk: the kept entries (lo, hi f32, row int32) of every
// segment, the segments' states (count, seen, T, flag), the settle's CSR
// (cidx int32, sim and key double, per kept entry).
inline size_t lshpc_user_bytes(int cap, int segs) { return (size_t)segs * ((size_t)cap * (12 + 4 + 16) + 16) + 64; }
// budget: LSHPC_BUDGET, or the test build's LSHKM_LSHPC_BUDGET=small (1 MiB:
// chunks of one user tile).
inline LshpcPlan lshpc_plan(int64_t N, int64_t nq, int P, int ncu, bool small_cap, size_t budget = LSHPC_BUDGET) {
    LshpcPlan p;
    p.cap = lshpc_cap(P, small_cap);
    const int64_t tiles = (nq + LSHPC_COLS - 1) / LSHPC_COLS;
    const int64_t by_rows = std::max<int64_t>(1, N / LSHPC_SEG_MIN);
    const int64_t by_fill = std::max<int64_t>(1, (LSHPC_FILL * (int64_t)std::max(ncu, 1) + tiles - 1) / tiles);
    p.segs = (int)std::min<int64_t>(LSHPC_SEG_MAX, std::min(by_rows, by_fill));
    const int64_t per = (N + p.segs - 1) / p.segs;
    p.seg_rows = std::max<int64_t>(LSHPC_STAGE, (per + LSHPC_STAGE - 1) / LSHPC_STAGE * LSHPC_STAGE);
    p.segs = (int)std::max<int64_t>(1, (N + p.seg_rows - 1) / p.seg_rows);
    const int64_t fit = (int64_t)(budget / lshpc_user_bytes(p.cap, p.segs));
    p.chunk = std::max<int64_t>(LSHPC_COLS, fit / LSHPC_COLS * LSHPC_COLS);
    if (p.chunk > nq) p.chunk = nq;
    return p;
}

// The chunk's workspace (n users, padded to whole tiles np): klo | khi (f32
// [np * segs][cap]) | krow (int32, same) | state (int32 [4][segs][np]: count,
// seen, T bits, flag) | nkept (int64 [n]) | cptr (int64 [n + 1]) | cidx (int32
// [n * segs * cap]) | sim | key (double, same) | replay (int32 [n]) | counts
// (uint32 [4]: replay, handed)
struct LshpcChunk {
    int64_t np;
    size_t klo, khi, krow, state, nkept, cptr, cidx, sim, key, replay, counts, bytes;
};
inline LshpcChunk lshpc_chunk(int64_t n, int cap, int segs) {
    LshpcChunk l;
    l.np = (n + LSHPC_COLS - 1) / LSHPC_COLS * LSHPC_COLS;
    const size_t e = (size_t)l.np * segs * cap, m = (size_t)std::max<int64_t>(n, 1);
    l.klo = 0;
    l.khi = l.klo + lshpc_round256(4 * e);
    l.krow = l.khi + lshpc_round256(4 * e);
    l.state = l.krow + lshpc_round256(4 * e);
    l.nkept = l.state + lshpc_round256(16 * (size_t)segs * l.np);
    l.cptr = l.nkept + lshpc_round256(8 * m);
    l.cidx = l.cptr + lshpc_round256(8 * (m + 1));
    l.sim = l.cidx + lshpc_round256(4 * e);
    l.key = l.sim + lshpc_round256(8 * e);
    l.replay = l.key + lshpc_round256(8 * e);
    l.counts = l.replay + lshpc_round256(4 * m);
    l.bytes = l.counts + 256;
    return l;
}

// ---- the lists path's chunks: candidate rows per chunk of handed-back users
// (~28 B of lists and workspace each), as lshkm_lsh_validate10 bounds its own.
constexpr int64_t LSHPC_CAND_CAP = (int64_t)1 << 28;

}  // namespace lshkm
