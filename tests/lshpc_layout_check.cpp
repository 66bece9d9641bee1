// Host check of csrc/lshpc_layout.h (tests/test_lshpc_layout_cpu.py): the
// routing rule's edges, the kept-list capacities, the row segments and user
// chunks of every plan, and the chunk workspace's regions.
#include <cstdio>

#include "../crypto-recommendation_amd/csrc/lshpc_layout.h"

using namespace lshkm;

static long bad = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) { bad++; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

int main() {
    // the rule: cosine, d <= 128, L * k <= 32, P + 1 + 64 <= 512
    CHECK(lshpc_route(true, 100, 5, 4, 20, false) == LshpcRoute::screen);
    CHECK(lshpc_route(true, 128, 1, 32, 447, false) == LshpcRoute::screen);
    CHECK(lshpc_route(true, 128, 1, 32, 448, false) == LshpcRoute::lists);
    CHECK(lshpc_route(true, 129, 5, 4, 20, false) == LshpcRoute::lists);
    CHECK(lshpc_route(true, 100, 11, 3, 20, false) == LshpcRoute::lists);
    CHECK(lshpc_route(false, 100, 5, 4, 20, false) == LshpcRoute::lists);
    CHECK(lshpc_route(true, 100, 5, 4, 20, true) == LshpcRoute::lists);
    CHECK(lshpc_dp(1) == 32 && lshpc_dp(32) == 32 && lshpc_dp(33) == 128 && lshpc_dp(128) == 128);
    for (int P = 1; P <= 447; P++) {
        for (int small = 0; small < 2; small++) {
            const int cap = lshpc_cap(P, small != 0);
            CHECK(cap >= lshpc_cap_min(P) && cap <= LSHPC_CAP_MAX);
            CHECK(small == 0 || cap == P + 1 + LSHPC_STAGE);
        }
    }
    const int64_t Ns[] = {1, 63, 64, 65, 300, 1061, 6000, 20000, 200000, 1000000, (1ll << 31) - 1};
    const int64_t nqs[] = {1, 127, 128, 129, 600, 20000, 200000, 1000000, (1ll << 31) - 1};
    for (int64_t N : Ns)
        for (int64_t nq : nqs)
            for (int P : {1, 20, 100, 447})
                for (int ncu : {0, 1, 256})
                    for (int small = 0; small < 2; small++)
                        for (size_t budget : {(size_t)1 << 20, LSHPC_BUDGET}) {
                            const LshpcPlan p = lshpc_plan(N, nq, P, ncu, small != 0, budget);
                            if (budget == LSHPC_BUDGET) {        // the default parameter is the product's budget
                                const LshpcPlan p0 = lshpc_plan(N, nq, P, ncu, small != 0);
                                CHECK(p0.cap == p.cap && p0.segs == p.segs && p0.seg_rows == p.seg_rows);
                                CHECK(p0.chunk == p.chunk);
                            }
                            CHECK(p.segs >= 1 && p.segs <= LSHPC_SEG_MAX);
                            CHECK(p.seg_rows % LSHPC_STAGE == 0 && p.seg_rows >= LSHPC_STAGE);
                            CHECK((int64_t)p.segs * p.seg_rows >= N);                  // the segments cover the rows
                            CHECK((int64_t)(p.segs - 1) * p.seg_rows < N);             // and none is empty
                            CHECK(p.chunk >= 1 && p.chunk <= nq);
                            CHECK(p.chunk == nq || p.chunk % LSHPC_COLS == 0);
                            const LshpcChunk c = lshpc_chunk(p.chunk, p.cap, p.segs);
                            CHECK(c.np >= p.chunk && c.np % LSHPC_COLS == 0 && c.np - p.chunk < LSHPC_COLS);
                            const size_t e = (size_t)c.np * p.segs * p.cap;
                            CHECK(c.khi >= c.klo + 4 * e && c.krow >= c.khi + 4 * e && c.state >= c.krow + 4 * e);
                            CHECK(c.nkept >= c.state + 16 * (size_t)p.segs * c.np);
                            CHECK(c.cptr >= c.nkept + 8 * (size_t)p.chunk);
                            CHECK(c.cidx >= c.cptr + 8 * (size_t)(p.chunk + 1));
                            CHECK(c.sim >= c.cidx + 4 * e && c.key >= c.sim + 8 * e && c.replay >= c.key + 8 * e);
                            CHECK(c.counts >= c.replay + 4 * (size_t)p.chunk && c.bytes >= c.counts + 16);
                            CHECK(c.sim % 8 == 0 && c.key % 8 == 0 && c.nkept % 8 == 0 && c.cptr % 8 == 0);
                            // the budget holds unless one tile of users alone exceeds it
                            CHECK(c.bytes <= budget + ((size_t)1 << 20) || p.chunk <= LSHPC_COLS);
                            // the chunks cover the users: whole chunks, then one smaller and not empty
                            const int64_t nchunks = (nq + p.chunk - 1) / p.chunk, last = nq - (nchunks - 1) * p.chunk;
                            CHECK(nchunks >= 1 && last >= 1 && last <= p.chunk && (nchunks - 1) * p.chunk + last == nq);
                            // a smaller last chunk fits the reservation made for the largest
                            CHECK(lshpc_chunk(last, p.cap, p.segs).bytes <= c.bytes);
                            CHECK(lshpc_chunk(1, p.cap, p.segs).bytes <= c.bytes);
                        }
    // the test build's 1 MiB budget (LSHKM_LSHPC_BUDGET=small): the shapes of
    // tests/test_gpu_lsh_closest_edges.py fall to one user tile per chunk
    for (int ncu : {1, 64, 256, 304}) {
        const size_t mib = (size_t)1 << 20;
        CHECK(lshpc_plan(6000, 600, 20, ncu, false, mib).chunk == LSHPC_COLS);
        CHECK(lshpc_plan(2000, 200, 15, ncu, false, mib).chunk == LSHPC_COLS);
        CHECK(lshpc_plan(1061, 130, 20, ncu, false, mib).chunk == LSHPC_COLS);
        CHECK(lshpc_plan(1061, 300, 20, ncu, false, mib).chunk == LSHPC_COLS);
        CHECK(lshpc_plan(6000, 600, 20, ncu, false).chunk == 600);
    }
    const LshpcImage im = lshpc_image(1061, 128, 5);
    CHECK(im.code >= 4 * (size_t)1061 * 128 && im.inv >= im.code + 4 * 1061 && im.rel >= im.inv + 4 * 1061);
    CHECK(im.xa >= im.rel + 4 * 1061 && im.xa % 8 == 0 && im.bucket >= im.xa + 8 * 1061);
    CHECK(im.bytes >= im.bucket + 4 * (size_t)1061 * 5);
    std::printf("bad=%ld\n", bad);
    return bad ? 1 : 0;
}
