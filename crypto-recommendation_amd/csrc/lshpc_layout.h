// lshpc_layout.h — the one statement of lshkm_lsh_p_closest's and
// lshkm_cube_p_closest's routing rules and of their workspaces: which calls the
// MFMA screen takes, the cube's candidacy test, the kept-list capacity, the row
// segments, the user chunks and every buffer's regions. Plain host arithmetic:
// no HIP (the candidacy test alone is also compiled for the device).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

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

// ---- lshkm_cube_p_closest: the same screen over a built hypercube. A row's
// code is its vertex, a user's code the vertex lshkm_cube_query gives it; row i
// is a candidate of user j iff vertex_i ^ vertex_j is one of the probe masks.
// Either metric (candidacy is by vertex alone, the similarity is cosine); the
// lists path: lshkm_cube_query's kernels -> lshkm_p_closest on the users handed
// back, gathered.
constexpr int LSHPC_CUBE_KMAX = 30;      // a vertex is a non-negative int32 (lshkm_cube_create's limit)
inline LshpcRoute cubepc_route(int d, int k, int P, bool force_lists) {
    if (force_lists || d > LSHPC_DMAX || k > LSHPC_CUBE_KMAX) return LshpcRoute::lists;
    return (int64_t)P + 1 + LSHPC_STAGE <= LSHPC_CAP_MAX ? LshpcRoute::screen : LshpcRoute::lists;
}

// Probe masks of get_hypercube_combined_buckets: 0 first (main bucket), then
// Hamming distance 1 (bit 0..k-1), 2 (lexicographic i<j), ... ; probes == 1
// starts at distance 2 (lsh_cube.hpp:148-150); stops when the cube is exhausted.
inline std::vector<int32_t> probe_masks(int probes, int k) {
    std::vector<int32_t> m(1, 0);
    int remaining = probes;
    int dist = probes > 1 ? 1 : 2;
    std::vector<int> comb(64);
    while (remaining > 0 && dist <= k) {
        for (int i = 0; i < dist; i++) comb[i] = i;
        for (;;) {
            int mask = 0;
            for (int i = 0; i < dist; i++) mask |= 1 << comb[i];
            m.push_back(mask);
            if (--remaining == 0) break;
            int p = dist - 1;
            while (p >= 0 && comb[p] == k - dist + p) p--;
            if (p < 0) break;
            comb[p]++;
            for (int q = p + 1; q < dist; q++) comb[q] = comb[q - 1] + 1;
        }
        dist++;
    }
    return m;
}

// Membership in probe_masks(probes, k) without the list. The masks after 0 run
// through the shells of popcount lo, lo + 1, ... (lo = 1, or 2 for probes == 1),
// each in lexicographic order of its ascending bit positions; with bit 0 first,
// that order is the descending order of the bit-reversed masks. So with `last`
// the popcount of the final mask and rev_last its bit reversal (0: the shell is
// whole), y is a mask iff y == 0, or popcount(y) in [lo, last), or popcount(y)
// == last and rev(y) >= rev_last. No mask after 0 (probes <= 0, k < lo): last
// = 0, which no popcount >= lo equals.
#if defined(__HIPCC__)
#define LSHPC_HD __host__ __device__
#else
#define LSHPC_HD
#endif
LSHPC_HD inline uint32_t cubepc_rev(uint32_t v) {
#if defined(__clang__)
    return __builtin_bitreverse32(v);
#else
    v = (v >> 16) | (v << 16);
    v = ((v & 0xff00ff00u) >> 8) | ((v & 0x00ff00ffu) << 8);
    v = ((v & 0xf0f0f0f0u) >> 4) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v & 0xccccccccu) >> 2) | ((v & 0x33333333u) << 2);
    return ((v & 0xaaaaaaaau) >> 1) | ((v & 0x55555555u) << 1);
#endif
}
struct CubeProbe {
    uint32_t shells;         // lo | last << 8
    uint32_t rev_last;
};
LSHPC_HD inline bool cubepc_member(uint32_t y, uint32_t shells, uint32_t rev_last) {
    const int p = __builtin_popcount(y), lo = (int)(shells & 0xffu), last = (int)(shells >> 8);
    // bitwise on purpose: the short-circuit form costs the kernel a branch per test
    return (y == 0u) | ((p >= lo) & ((p < last) | ((p == last) & (cubepc_rev(y) >= rev_last))));
}
inline int64_t cubepc_choose(int n, int r) {
    if (r < 0 || r > n) return 0;
    int64_t c = 1;
    for (int i = 1; i <= r; i++) c = c * (n - r + i) / i;        // exact: C(n - r + i, i) at every step
    return c;
}
inline CubeProbe cubepc_probe(int probes, int k) {
    const int lo = probes > 1 ? 1 : 2;
    int64_t remaining = probes;
    int last = 0;
    uint32_t rev_last = 0;
    for (int dist = lo; remaining > 0 && dist <= k; dist++) {
        const int64_t shell = cubepc_choose(k, dist);
        last = dist;
        rev_last = 0;
        if (remaining >= shell) {
            remaining -= shell;
            continue;
        }
        // the shell's combination of lexicographic rank remaining - 1
        int64_t r = remaining - 1;
        uint32_t mask = 0;
        for (int i = 0, c = 0; i < dist; i++, c++) {
            for (;; c++) {
                const int64_t with_c = cubepc_choose(k - 1 - c, dist - 1 - i);
                if (r < with_c) break;
                r -= with_c;
            }
            mask |= 1u << c;
        }
        rev_last = cubepc_rev(mask);
        remaining = 0;
    }
    return CubeProbe{(uint32_t)lo | (uint32_t)last << 8, rev_last};
}

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
