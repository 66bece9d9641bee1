// Host check of csrc/recom_layout.h: over S x nq x nitems x nusers x row sizes,
// the regions of each workspace are in order, disjoint, aligned and inside the
// reservation; the item and user records are 16-B aligned from a 256-B aligned
// base; recom_route says terms exactly for rows of a multiple of 8 B up to
// 1016 B with at most 2^28 terms, and every LDS size it implies fits 160 KiB;
// the long-user batches are contiguous, cover the list and keep both limits
// unless a batch is a single user; the wave form's scratch keeps its bound; the
// cluster-major work list is what its layout says. Prints "bad=0" and exits 0
// when all hold.
#include <cstdio>
#include <initializer_list>
#include <utility>
#include <vector>

#include "../crypto-recommendation_amd/csrc/recom_layout.h"

using namespace lshkm;

static long bad = 0, checked = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        checked++;                                                      \
        if (!(c)) {                                                     \
            if (bad++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
        }                                                               \
    } while (0)

// regions {offset, bytes, alignment} of one buffer of `bytes`: in the listed
// order, each aligned, none overlapping the next, the last inside the buffer
struct Region {
    size_t off, len, align;
};
static void in_order(size_t bytes, std::initializer_list<Region> rs) {
    size_t end = 0;
    for (const Region& r : rs) {
        CHECK(r.off >= end);
        CHECK(r.off % r.align == 0);
        end = r.off + r.len;
    }
    CHECK(end <= bytes);
}

static void check_map(int64_t S, int64_t nq) {
    const RcMapLayout l = rc_map_layout(S, nq);
    const size_t s = (size_t)S, q = (size_t)nq;
    in_order(l.bytes, {{l.mq, 4 * s, 4}, {l.mr, 4 * s, 4}, {l.fix_list, 8 * s, 8}, {l.fix_count, 8, 8},
                       {l.unorm, 8 * q, 8}, {l.fix_region, 8 * s, 8}, {l.fix_aux, 16 * (size_t)RC_TERMS_GMAX, 8}});
}

static void check_pack(size_t pack_len, int64_t nitems, int64_t nusers) {
    const RcPackLayout l = rc_pack_layout(pack_len, nitems, nusers);
    in_order(l.bytes, {{l.pack, 4 * pack_len, 4}, {l.items, RC_ITEM_BYTES * (size_t)nitems, 16},
                       {l.users, RC_USER_BYTES * (size_t)nusers, 16}});
    for (const size_t base : {(size_t)0, (size_t)256, (size_t)0x7f00}) {     // 256-B aligned bases
        CHECK((base + l.items) % 16 == 0 && (base + l.users) % 16 == 0);
    }
    CHECK(RC_ITEM_BYTES % 16 == 0 && RC_USER_BYTES % 16 == 0);               // every record, not only the first
}

static void check_long(int64_t rows, int64_t nl, int64_t D, size_t seg_ws) {
    const RcLongLayout l = rc_long_layout(rows, nl, D, seg_ws);
    const size_t v = (size_t)rows * D * 8, c = (size_t)nl * D * 8;
    in_order(l.bytes, {{l.ws, seg_ws, 256}, {l.V, v, 8}, {l.carry, c, 8}, {l.sums, c, 8},
                       {l.tab, (size_t)nl * sizeof(RcLongUser), 8}, {l.crow, (size_t)(nl + 1) * 8, 8},
                       {l.iota, (size_t)rows * 4, 4}});
}

static void check_route() {
    const int64_t cap = (int64_t)1 << 28;
    for (int rb = 4; rb <= 1200; rb += 4)
        for (const bool f64 : {false, true}) {
            const int elem = f64 ? 8 : 4;
            if (rb % elem) continue;
            const int d = rb / elem;
            const bool rows = rb % 8 == 0 && rb <= 1016;
            for (const int64_t t : {(int64_t)0, (int64_t)1, cap, cap + 1, (int64_t)1 << 40}) {
                const RecomRoute want = rows && t <= cap ? RecomRoute::terms : RecomRoute::waves;
                CHECK(recom_route(d, f64, t) == want);
            }
            if (rows) {
                const int s8 = rc_terms_stride8(d, elem);
                CHECK((int64_t)s8 * 8 >= rb + 8);                          // the row and a spare unit
                CHECK(rc_terms_lds_fix(s8) <= 160 * 1024 && rc_terms_lds_cl(s8) <= 160 * 1024);
                CHECK(rc_terms_lds_cl(s8) >= (size_t)(CT_STAGE + CT_UMAX + 1) * (size_t)rb);
            }
        }
    // the edges by name: 1016 / 1024 B rows of both types, 2^28 / 2^28 + 1 terms
    CHECK(recom_route(254, false, cap) == RecomRoute::terms && recom_route(256, false, 0) == RecomRoute::waves);
    CHECK(recom_route(127, true, cap) == RecomRoute::terms && recom_route(128, true, 0) == RecomRoute::waves);
    CHECK(recom_route(128, false, cap) == RecomRoute::terms && recom_route(128, false, cap + 1) == RecomRoute::waves);
    CHECK(recom_route(2, false, 0) == RecomRoute::terms && recom_route(1, false, 0) == RecomRoute::waves);
    CHECK(recom_route(0, false, 0) == RecomRoute::refused && recom_route(8, true, -1) == RecomRoute::refused);
}

static void check_batches(const std::vector<RcLongUser>& lus) {
    const std::vector<RcLongBatch> bs = rc_long_batches(lus);
    size_t next = 0;
    for (const RcLongBatch& b : bs) {
        CHECK(b.k0 == next && b.k1 > b.k0 && b.k1 <= lus.size());        // contiguous, non-empty
        int64_t rows = 0, D = 1;
        for (size_t k = b.k0; k < b.k1; k++) {
            rows += lus[k].n;
            D = std::max<int64_t>(D, lus[k].m + 1);
        }
        CHECK(rows == b.rows && D == b.D);
        if (b.k1 - b.k0 > 1) CHECK(b.rows * b.D * 8 <= RC_LONG_VALUE_BYTES && b.rows < RC_LONG_ROWS);
        // greedy: the next user would not have fitted
        if (b.k1 < lus.size()) {
            const int64_t r2 = rows + lus[b.k1].n, D2 = std::max<int64_t>(D, lus[b.k1].m + 1);
            CHECK(r2 * D2 * 8 > RC_LONG_VALUE_BYTES || r2 >= RC_LONG_ROWS);
        }
        next = b.k1;
    }
    CHECK(next == lus.size());                                             // covers the list
    CHECK(bs.empty() == lus.empty());
}

static RcLongUser lu(int64_t n, int64_t m) { return RcLongUser{0, n, 0, 0, 0, m, 0, 0}; }

static void check_work_list() {
    // users 0..6 of clusters 2, 0, 2, 1 (no member here), 0, 2, 5; members 64, 65, 64, 0, 65, 64, 1
    const std::vector<int32_t> hu = {2, 0, 2, 1, 0, 2, 5};
    const std::vector<int64_t> soff = {0, 64, 129, 193, 193, 258, 322, 323};
    const RcWorkList w = rc_work_list(hu, soff);
    CHECK(w.ngroups == 3 && w.nusers == 6 && w.nitems == 2 + 1 + 1);
    const std::vector<int32_t> want = {0, 2, 3, 4, /* gcl */ 0, 2, 5, /* gptr */ 0, 2, 5, 6, /* gusr */ 1, 4, 0, 2, 5, 6};
    CHECK(w.pack == want);
    CHECK(w.gcl() == 4 && w.gptr() == 7 && w.gusr() == 11 && w.pack.size() == w.gusr() + (size_t)w.nusers);
    const RcWorkList e = rc_work_list({}, {0});
    CHECK(e.ngroups == 0 && e.nitems == 0 && e.nusers == 0);
}

int main() {
    const int64_t Ss[] = {0, 1, 63, 64, 65, 2147483647};
    const int64_t nqs[] = {1, 2, 8191, 8192, 8193, 65537};
    const int64_t cnt[] = {1, 2, 4097};
    for (const int64_t S : Ss)
        for (const int64_t nq : nqs) {
            check_map(S, nq);
            CHECK(rc_map_layout(S, nq).bytes == 24 * (size_t)S + 16 + 8 * (size_t)nq + 16 * (size_t)RC_TERMS_GMAX);
        }
    for (const int64_t ni : cnt)
        for (const int64_t nu : cnt)
            for (const int64_t G : {(int64_t)1, nu}) check_pack((size_t)(3 * G + 2 + nu), ni, nu);
    for (const int64_t rows : {RC_LONG_MIN, (int64_t)100001, (int64_t)2147483647})
        for (const int64_t nl : cnt)
            for (const int64_t D : {(int64_t)1, (int64_t)2, (int64_t)255})
                for (const size_t ws : {(size_t)0, (size_t)1, (size_t)4097}) check_long(rows, nl, D, ws);
    check_route();
    // batches: a single user over 1 GiB of values alone and between others; many
    // users of RC_LONG_MIN members; a sum of rows crossing 2^31; m = 0
    check_batches({});
    check_batches({lu(RC_LONG_MIN, 0)});
    check_batches({lu((int64_t)1 << 28, 7)});
    check_batches({lu(RC_LONG_MIN, 3), lu((int64_t)1 << 28, 7), lu(RC_LONG_MIN, 3)});
    check_batches(std::vector<RcLongUser>(5000, lu(RC_LONG_MIN, 9)));
    check_batches(std::vector<RcLongUser>(40, lu(((int64_t)1 << 26) - 1, 0)));      // 8 B a row: two users a batch
    check_batches({lu(((int64_t)1 << 31) - 1, 0), lu(1, 0), lu(RC_LONG_MIN, 300), lu(RC_LONG_MIN, 0)});   // 2^31 rows
    {
        std::vector<RcLongUser> mixed;
        for (int i = 0; i < 3000; i++) mixed.push_back(lu(RC_LONG_MIN + (int64_t)i * 7919 % 900000, i % 257));
        check_batches(mixed);
    }
    // the wave form's scratch: whole blocks, at most 1 GiB unless one block needs more
    for (const int64_t nq : nqs)
        for (const int64_t mx : {(int64_t)0, (int64_t)1, (int64_t)65, (int64_t)1 << 20, (int64_t)2147483647}) {
            const RcWaveScratch w = rc_wave_scratch(nq, mx);
            CHECK(w.row == std::max<int64_t>(mx, 1) && w.row >= mx);
            CHECK(w.nwaves >= 1 && w.nwaves % RC_CLUSTER_WAVES_PER_BLOCK == 0 && w.nwaves <= 8192);
            CHECK(w.bytes == (size_t)w.nwaves * (size_t)w.row * 8);
            CHECK(w.bytes <= (size_t)RC_WAVE_SCRATCH_BYTES || w.nwaves == RC_CLUSTER_WAVES_PER_BLOCK);
            CHECK(w.nwaves < nq + RC_CLUSTER_WAVES_PER_BLOCK);
        }
    check_work_list();
    printf("checked=%ld bad=%ld\n", checked, bad);
    return bad ? 1 : 0;
}
