// recom_layout.h — the one statement of the clustering recommender's form rule
// and of its workspaces: which rows the terms form runs, every buffer's regions
// and size, the batches of the long-cluster chains, the wave form's scratch and
// the cluster-major work list. Plain host arithmetic: no HIP
// (tests/recom_layout_check.cpp includes it as it is).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lshkm {

// ---- the form rule. terms: every (member, user) pair at once from rows staged
// in LDS in 8-B units, then the chains from the stored terms; waves: one wave
// per user. The terms form needs rows of a multiple of 8 B up to RC_ROW_MAX
// that stage within the LDS, and at most RC_TERMS_MAX terms (2 GiB of doubles).
constexpr int CT_STAGE = 64;         // member rows staged per wave
constexpr int CT_UMAX = 4;           // users per item staged ahead
constexpr int64_t RC_ROW_MAX = 1016, RC_TERMS_MAX = 1ll << 28;
constexpr size_t RC_LDS_BYTES = 160 * 1024;
inline int rc_terms_stride8(int d, int elem) { return (int)(((int64_t)d * elem + 7) / 8) + 1; }
// rc_terms_fix_kernel: the rows and a spare, twice; rc_terms_cl_kernel: rows | the users' rows | a spare
inline size_t rc_terms_lds_fix(int stride8) { return 2 * (size_t)(CT_STAGE + 1) * stride8 * 8; }
inline size_t rc_terms_lds_cl(int stride8) { return (size_t)(CT_STAGE + CT_UMAX + 1) * stride8 * 8; }
enum class RecomRoute { terms, waves, refused };
inline RecomRoute recom_route(int d, bool f64, int64_t terms_total) {
    if (d < 1 || terms_total < 0) return RecomRoute::refused;
    const int elem = f64 ? 8 : 4;
    const int64_t rb = (int64_t)d * elem;
    if (rb % 8 != 0 || rb > RC_ROW_MAX || terms_total > RC_TERMS_MAX) return RecomRoute::waves;
    const int stride8 = rc_terms_stride8(d, elem);
    return rc_terms_lds_fix(stride8) <= RC_LDS_BYTES && rc_terms_lds_cl(stride8) <= RC_LDS_BYTES ? RecomRoute::terms
                                                                                               : RecomRoute::waves;
}

inline size_t rc_round256(size_t b) { return (b + 255) / 256 * 256; }

// ---- member map of the terms form (S = soff[nq] members): mq | mr (int32 [S]
// each: member -> user, row) | the declined-member list (int64 [S]) | its count
// (u64) | the users' |u|^2 (double [nq]) | the blocks' private decline lists
// (int64 [S]) | their capacities and counts (int64 [2][RC_TERMS_GMAX])
constexpr int RC_TERMS_GMAX = 8192;
struct RcMapLayout {
    size_t mq, mr, fix_list, fix_count, unorm, fix_region, fix_aux, bytes;
};
inline RcMapLayout rc_map_layout(int64_t S, int64_t nq) {
    const size_t s = (size_t)S, q = (size_t)nq;
    RcMapLayout l;
    l.mq = 0;
    l.mr = 4 * s;
    l.fix_list = 8 * s;
    l.fix_count = l.fix_list + 8 * s;
    l.unorm = l.fix_count + 8;
    l.fix_region = l.unorm + 8 * q;
    l.fix_aux = l.fix_region + 8 * s;
    l.bytes = 24 * s + 16 + 8 * q + 16 * (size_t)RC_TERMS_GMAX;
    return l;
}

// ---- cluster-major work list of the terms form (rc_terms_cl_kernel): group g =
// the users gusr[gptr[g] .. gptr[g + 1]) of cluster gcl[g] (ascending) with
// members on this shard; the 64-member chunks of the cluster's rows are the
// items ioff[g] .. ioff[g + 1] - 1, each staged once for all of the group's
// users. pack: ioff [G + 1] | gcl [G] | gptr [G + 1] | gusr [nusers].
struct RcWorkList {
    std::vector<int32_t> pack;
    int ngroups = 0;
    int64_t nitems = 0, nusers = 0;
    size_t gcl() const { return (size_t)ngroups + 1; }       // int32 offsets in pack
    size_t gptr() const { return 2 * (size_t)ngroups + 1; }
    size_t gusr() const { return 3 * (size_t)ngroups + 2; }
};
inline RcWorkList rc_work_list(const std::vector<int32_t>& hu, const std::vector<int64_t>& soff) {
    const int64_t nq = (int64_t)hu.size();
    std::vector<int32_t> byc;
    byc.reserve((size_t)nq);
    for (int64_t q = 0; q < nq; q++)
        if (soff[q + 1] > soff[q]) byc.push_back((int32_t)q);
    std::stable_sort(byc.begin(), byc.end(), [&](int32_t a, int32_t b) { return hu[a] < hu[b]; });
    std::vector<int32_t> gcl, gptr(1, 0), ioff(1, 0);
    for (size_t k = 0; k < byc.size(); k++) {
        const int32_t q = byc[k];
        if (k == 0 || hu[q] != hu[byc[k - 1]]) {
            if (k) gptr.push_back((int32_t)k);
            gcl.push_back(hu[q]);
            ioff.push_back(ioff.back() + (int32_t)((soff[q + 1] - soff[q] + CT_STAGE - 1) / CT_STAGE));
        }
    }
    gptr.push_back((int32_t)byc.size());
    RcWorkList w;
    w.ngroups = (int)gcl.size();
    w.nitems = w.ngroups ? (int64_t)ioff.back() : 0;
    w.nusers = (int64_t)byc.size();
    w.pack.reserve(w.gusr() + byc.size());
    for (const auto* v : {&ioff, &gcl, &gptr, &byc}) w.pack.insert(w.pack.end(), v->begin(), v->end());
    return w;
}
// its device buffer: the pack, then the per-item and per-user records
// (rc_item_meta_kernel, rc_user_meta_kernel: 16-B aligned), each from a 256-B boundary
constexpr size_t RC_ITEM_BYTES = 32, RC_USER_BYTES = 48;
struct RcPackLayout {
    size_t pack, items, users, bytes;
};
inline RcPackLayout rc_pack_layout(size_t pack_len, int64_t nitems, int64_t nusers) {
    RcPackLayout l;
    l.pack = 0;
    l.items = rc_round256(4 * std::max<size_t>(pack_len, 1));
    l.users = l.items + rc_round256(RC_ITEM_BYTES * (size_t)std::max<int64_t>(nitems, 1));
    l.bytes = l.users + RC_USER_BYTES * (size_t)std::max<int64_t>(nusers, 1);
    return l;
}

// ---- users whose cluster holds >= RC_LONG_MIN members on this shard: their
// prediction chains by binade segments (launch_seg_columns, all users of a batch
// in one set of launches) instead of one wave's sequential adds.
constexpr int64_t RC_LONG_MIN = 16384;
struct RcLongUser {
    int64_t q, n, b0, toff, u0, m, off, pad;     // off: the user's first row in its batch's V
};
// A batch: users [k0, k1), D = their max m + 1 columns (each user's terms,
// zero-padded, then |sim|) over rows = their members: rows * D * 8 <=
// RC_LONG_VALUE_BYTES and rows < RC_LONG_ROWS, one user at least.
constexpr int64_t RC_LONG_VALUE_BYTES = 1ll << 30, RC_LONG_ROWS = 1ll << 31;
struct RcLongBatch {
    size_t k0, k1;
    int64_t rows, D;
};
inline std::vector<RcLongBatch> rc_long_batches(const std::vector<RcLongUser>& lus) {
    std::vector<RcLongBatch> out;
    for (size_t k0 = 0; k0 < lus.size();) {
        RcLongBatch b{k0, k0, 0, 1};
        while (b.k1 < lus.size()) {
            const int64_t D2 = std::max<int64_t>(b.D, lus[b.k1].m + 1), rows2 = b.rows + lus[b.k1].n;
            if (b.k1 > k0 && (rows2 * D2 * 8 > RC_LONG_VALUE_BYTES || rows2 >= RC_LONG_ROWS)) break;
            b.D = D2;
            b.rows = rows2;
            b.k1++;
        }
        out.push_back(b);
        k0 = b.k1;
    }
    return out;
}
// its device workspace (nl users): ws (launch_seg_columns' own, seg_ws_bytes) |
// V [rows][D] | carry, sums [nl][D] | tab [nl] RcLongUser | crow [nl + 1] (row
// offsets in V) | iota [rows] int32
struct RcLongLayout {
    size_t ws, V, carry, sums, tab, crow, iota, bytes;
};
inline RcLongLayout rc_long_layout(int64_t rows, int64_t nl, int64_t D, size_t seg_ws_bytes) {
    const size_t cb = (size_t)nl * (size_t)D * 8;
    RcLongLayout l;
    l.ws = 0;
    l.V = rc_round256(seg_ws_bytes);
    l.carry = l.V + (size_t)rows * (size_t)D * 8;
    l.sums = l.carry + cb;
    l.tab = l.sums + cb;
    l.crow = l.tab + (size_t)nl * sizeof(RcLongUser);
    l.iota = l.crow + (size_t)(nl + 1) * 8;
    l.bytes = l.iota + (size_t)rows * 4 + 256;
    return l;
}

// ---- the wave form (rc_cluster_top_n_kernel): one wave per user in flight, the
// scratch row of a wave holds one cluster's similarities (row = the largest
// cluster); at most RC_WAVE_SCRATCH_BYTES of scratch (fewer waves for huge
// clusters, one block at least), a whole number of blocks
constexpr int RC_CLUSTER_WAVES_PER_BLOCK = 4;     // RC_WAVES
constexpr int64_t RC_WAVE_SCRATCH_BYTES = 1ll << 30;
struct RcWaveScratch {
    int64_t row;
    int nwaves;
    size_t bytes;
};
inline RcWaveScratch rc_wave_scratch(int64_t nq, int64_t max_members) {
    const int64_t W = RC_CLUSTER_WAVES_PER_BLOCK, row = std::max<int64_t>(max_members, 1);
    int64_t nw = std::min<int64_t>(nq, 8192);
    nw = std::min<int64_t>(nw, std::max<int64_t>(W, RC_WAVE_SCRATCH_BYTES / (row * 8)));
    nw = (nw + W - 1) / W * W;
    return {row, (int)nw, sizeof(double) * (size_t)nw * (size_t)row};
}

}  // namespace lshkm
