// Host check of csrc/knn_layout.h (tests/test_knn_cpu.py compiles and runs it,
// once plain and once under the host sanitizers): the plan's group and segment
// arithmetic, the route, the workspace regions, and the threshold rule itself
// on random intervals.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../crypto-recommendation_amd/csrc/knn_layout.h"

using namespace lshkm;

static int bad = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            bad++;                                            \
            printf("line %d: %s\n", __LINE__, #c);            \
        }                                                     \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}
static double unit() { return (double)rnd() / (double)(1ull << 31); }

// The rule of DESIGN.md 5g on n values in groups of grp: tau = the k-th
// smallest of the groups' smallest hi; every one of the k smallest values (by
// value, then index) must have lo <= tau. Returns the rows with lo <= tau, or
// -1 when the rule has fewer than k groups.
static int threshold_rule(int n, int grp, int k, double width, bool ties) {
    std::vector<double> v(n), lo(n), hi(n);
    for (int i = 0; i < n; i++) {
        v[i] = ties ? (double)(rnd() % 8) : unit();
        lo[i] = v[i] - width * unit();
        hi[i] = v[i] + width * unit();
    }
    const int groups = (n + grp - 1) / grp;
    if (groups < k) return -1;
    std::vector<double> gmin(groups, 1e300);
    for (int i = 0; i < n; i++) gmin[i / grp] = std::min(gmin[i / grp], hi[i]);
    std::sort(gmin.begin(), gmin.end());
    const double tau = gmin[k - 1];
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return v[a] < v[b] || (v[a] == v[b] && a < b); });
    for (int j = 0; j < k; j++) CHECK(lo[order[j]] <= tau);
    int kept = 0;
    for (int i = 0; i < n; i++) kept += lo[i] <= tau;
    CHECK(kept >= k);
    return kept;
}

int main() {
    // limits and capacities
    CHECK(KNN_KMAX == 64 && KNN_GRP_MIN == 32 && KNN_GROUPS_MAX % 64 == 0);
    for (int k = 1; k <= KNN_KMAX; k++) {
        CHECK(knn_cap(k, true) == k && knn_cap(k, false) >= k + 32 && knn_cap(k, false) <= KNN_CAP_MAX);
    }
    // route: d 128 / 129, forced, groups k - 1 / k, poison rows 16 / 17, real rows k - 1 / k
    CHECK(knn_route(1, 1, 1, false) == KnnRoute::screen);
    CHECK(knn_route(128, 10, 10, false) == KnnRoute::screen);
    CHECK(knn_route(129, 10, 10, false) == KnnRoute::scan);
    CHECK(knn_route(128, 10, 9, false) == KnnRoute::scan);
    CHECK(knn_route(128, 1, 0, false) == KnnRoute::scan);
    CHECK(knn_route(20, 1, 100, true) == KnnRoute::scan);
    CHECK(knn_route_after_prep(100, 10, 0) == KnnRoute::screen);
    CHECK(knn_route_after_prep(100, 10, NEAREST_POISON_MAX) == KnnRoute::screen);
    CHECK(knn_route_after_prep(100, 10, NEAREST_POISON_MAX + 1) == KnnRoute::scan);
    CHECK(knn_route_after_prep(20, 10, 10) == KnnRoute::screen);
    CHECK(knn_route_after_prep(20, 10, 11) == KnnRoute::scan);

    // the plan over (N, nq, k, CU count, switches)
    const int64_t Ns[] = {1, 31, 32, 33, 63, 64, 65, 200, 1023, 1024, 1025, 2047, 2048, 4096, 4097, 32768, 32769,
                          100000, 1000000, (1ll << 31) - 1};
    const int64_t nqs[] = {1, 127, 128, 129, 4096, 20000, 32768, 32769, 1 << 20, 1 << 25, (1 << 25) + 1, (1ll << 31) - 1};
    const int ks[] = {1, 2, 10, 63, 64};
    for (int64_t N : Ns)
        for (int64_t nq : nqs)
            for (int k : ks)
                for (int sw = 0; sw < 4; sw++)
                    for (int ncu : {1, 256}) {
                        const bool small_cap = sw & 1, small_seg = sw & 2;
                        const KnnPlan p = knn_plan(N, nq, k, ncu, small_cap, small_seg);
                        CHECK(p.cap == knn_cap(k, small_cap) && p.cap >= k);
                        CHECK(p.tiles * NEAREST_COLS >= nq && (p.tiles - 1) * NEAREST_COLS < nq);
                        // groups: whole MFMA tiles, disjoint ranges [g grp_rows, (g + 1) grp_rows) that cover [0, N)
                        CHECK(p.grp_rows == (int64_t)1 << p.grp_shift && p.grp_rows % KNN_GRP_MIN == 0);
                        if (small_seg) CHECK(p.grp_rows >= NEAREST_STAGE);
                        CHECK(p.groups >= 0 && p.groups <= KNN_GROUPS_MAX);
                        CHECK((int64_t)p.groups * nq <= KNN_KEYS_MAX);                   // the key array's bound
                        if (p.groups > 0) {
                            CHECK((int64_t)p.groups * p.grp_rows >= N && (int64_t)(p.groups - 1) * p.grp_rows < N);
                        } else {
                            CHECK(nq > KNN_KEYS_MAX);
                        }
                        // as fine as the bounds allow: half the group size would break one of them
                        if (p.groups > 0 && p.grp_rows > (small_seg ? NEAREST_STAGE : KNN_GRP_MIN)) {
                            const int64_t finer = (N + p.grp_rows / 2 - 1) / (p.grp_rows / 2);
                            CHECK(finer > KNN_GROUPS_MAX || finer * nq > KNN_KEYS_MAX);
                        }
                        // segments: whole groups and whole stages, cover the rows, none empty, a legal grid
                        CHECK(p.segs >= 1 && p.segs <= NEAREST_SEG_MAX && p.segs <= 65535);
                        CHECK(p.seg_rows % NEAREST_STAGE == 0 && p.seg_rows % p.grp_rows == 0);
                        CHECK((int64_t)p.segs * p.seg_rows >= N && (int64_t)(p.segs - 1) * p.seg_rows < N);
                        // the route goes to the scan wherever the rule lacks k groups
                        if (p.groups < k) CHECK(knn_route(1, k, p.groups, false) == KnnRoute::scan);
                        else CHECK(knn_route(1, k, p.groups, false) == KnnRoute::screen);
                    }
    // the default grain: 32-row groups up to 32,768 rows; N = 4,096 makes 128 groups
    CHECK(knn_plan(4096, 256, 10, 256, false, false).groups == 128);
    CHECK(knn_plan(4097, 256, 10, 256, false, false).groups == 129);
    CHECK(knn_plan(32768, 1, 1, 256, false, false).grp_rows == 32);
    CHECK(knn_plan(32769, 1, 1, 256, false, false).grp_rows == 64);
    CHECK(knn_plan(1000000, 4096, 64, 256, false, false).groups == 977);
    CHECK(knn_plan(1000000, 4096, 64, 256, false, false).grp_rows == 1024);
    CHECK(knn_plan(200000, 20000, 64, 256, false, false).groups == 782);
    // small segments: one stage per group and per segment
    CHECK(knn_plan(300, 1, 2, 256, false, true).groups == 5 && knn_plan(300, 1, 2, 256, false, true).segs == 5);
    CHECK(knn_plan(300, 1, 2, 256, false, true).seg_rows == 64);
    CHECK(knn_plan(64, 1, 1, 256, false, true).segs == 1 && knn_plan(65, 1, 1, 256, false, true).segs == 2);

    // regions: ordered, aligned, disjoint, inside bytes
    for (int64_t nq : {0ll, 1ll, 129ll, 20000ll})
        for (int groups : {0, 1, 129, KNN_GROUPS_MAX})
            for (int cap : {1, 64, KNN_CAP_MAX}) {
                const KnnState s = knn_state(nq, groups, cap);
                const size_t m = nq > 0 ? (size_t)nq : 1, g = groups > 0 ? (size_t)groups : 1;
                CHECK(s.gkey == 0 && s.tau >= 4 * m * g && s.cnt >= s.tau + 4 * m && s.krow >= s.cnt + 4 * m);
                CHECK(s.scan >= s.krow + 4 * m * cap && s.pois >= s.scan + 4 * m);
                CHECK(s.counts >= s.pois + 4 * (size_t)NEAREST_POISON_MAX && s.bytes >= s.counts + 16);
                CHECK(s.tau % 256 == 0 && s.cnt % 256 == 0 && s.krow % 256 == 0 && s.scan % 256 == 0 &&
                      s.pois % 256 == 0 && s.counts % 256 == 0);
            }

    // the threshold rule on random intervals: narrow, wide, and with exact ties
    long kept_sum = 0, runs = 0;
    for (int trial = 0; trial < 400; trial++) {
        const int n = 1 + (int)(rnd() % 3000), grp = 32 << (rnd() % 3), k = 1 + (int)(rnd() % 64);
        const double width = trial % 3 == 0 ? 1e-6 : trial % 3 == 1 ? 1e-2 : 0.5;
        const int kept = threshold_rule(n, grp, k, width, trial % 5 == 0);
        if (kept >= 0 && trial % 3 == 0 && trial % 5 != 0 && n >= 64 * grp) {
            kept_sum += kept - k;
            runs++;
        }
    }
    CHECK(threshold_rule(100, 32, 5, 0.1, false) == -1);      // 4 groups: the scan's
    printf("narrow intervals, >= 64 groups: %.2f rows kept beyond k on average over %ld runs\n",
           runs ? (double)kept_sum / runs : 0.0, runs);
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
