// Host check of csrc/pair_merge.h against a sort, exhaustively over small
// integer-valued scores (so ties of every kind occur):
//  - top3_insert over every sequence of up to 7 scores from {0..3}, two scores
//    per tile: the three values are the sequence's largest three, (m1, t1) and
//    (m2, t2) are two different scores with their own tiles, and t1 is the
//    first tile that reaches the maximum (tile_epilogue's rule);
//  - merge_halves over every pair of halves of 3 and 4 scores from {0..3}: I2
//    is a centroid other than I1 with the second-largest score, and M3 is the
//    largest score of all the others (so it bounds them).
// Prints "bad=0" and exits 0 when all hold.
#include <algorithm>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "../crypto-recommendation_amd/csrc/pair_merge.h"

using namespace lshkm;

static long bad = 0, checked = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        checked++;                                                      \
        if (!(c)) {                                                     \
            if (bad++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
        }                                                               \
    } while (0)

static const float NINF = -std::numeric_limits<float>::infinity();

static void check_insert(const std::vector<int>& seq) {
    Top3 s = {NINF, NINF, NINF, 0, 0};
    for (size_t p = 0; p < seq.size(); p++) top3_insert(s, (float)seq[p], (int)(p / 2));
    std::vector<float> v(seq.begin(), seq.end());
    v.resize(std::max<size_t>(v.size(), 3), NINF);
    std::sort(v.begin(), v.end(), std::greater<float>());
    CHECK(s.m1 == v[0] && s.m2 == v[1] && s.m3 == v[2]);
    // two different positions p1 != p2 with (value, tile) = (m1, t1) and (m2, t2)
    bool found = seq.size() < 2;
    for (size_t p1 = 0; p1 < seq.size() && !found; p1++)
        for (size_t p2 = 0; p2 < seq.size() && !found; p2++)
            found = p1 != p2 && (float)seq[p1] == s.m1 && (int)(p1 / 2) == s.t1 && (float)seq[p2] == s.m2 &&
                    (int)(p2 / 2) == s.t2;
    CHECK(found);
    size_t first = 0;
    while (first < seq.size() && (float)seq[first] != v[0]) first++;
    if (!seq.empty()) CHECK(s.t1 == (int)(first / 2));
}

// a half's state from its scores: score p of half h is centroid 2 p + h
static HalfTop half_of(const std::vector<int>& sc, int h) {
    std::vector<int> idx(sc.size());
    for (size_t p = 0; p < sc.size(); p++) idx[p] = (int)p;
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return sc[x] > sc[y]; });
    return {(float)sc[idx[0]], (float)sc[idx[1]], (float)sc[idx[2]], 2 * idx[0] + h, 2 * idx[1] + h};
}

static void check_merge(const std::vector<int>& a, const std::vector<int>& b) {
    const HalfTop me = half_of(a, 0), ot = half_of(b, 1);
    // the kernel's winner: the larger m1, the smaller index on a tie
    const bool other = ot.m1 > me.m1 || (ot.m1 == me.m1 && ot.i1 < me.i1);
    const int I1 = other ? ot.i1 : me.i1;
    const PairMerge pm = other ? merge_halves(ot, me) : merge_halves(me, ot);
    std::vector<float> all;
    float rest = NINF, s2 = NINF;
    bool named = false;
    for (size_t p = 0; p < a.size() + b.size(); p++) {
        const int h = p < a.size() ? 0 : 1;
        const size_t q = h ? p - a.size() : p;
        const int c = 2 * (int)q + h;
        const float v = (float)(h ? b[q] : a[q]);
        all.push_back(v);
        if (c == pm.I2) { named = true; s2 = v; }
        if (c != I1 && c != pm.I2) rest = std::max(rest, v);
    }
    std::sort(all.begin(), all.end(), std::greater<float>());
    CHECK(named && pm.I2 != I1);
    CHECK(s2 == all[1]);
    CHECK(pm.M3 == rest && pm.M3 == all[2]);
}

static void each_seq(int len, const std::function<void(const std::vector<int>&)>& f) {
    std::vector<int> s(len, 0);
    for (;;) {
        f(s);
        int p = 0;
        while (p < len && ++s[p] == 4) s[p++] = 0;
        if (p == len) return;
    }
}

int main() {
    for (int len = 0; len <= 7; len++) each_seq(len, check_insert);
    for (const int la : {3, 4})
        for (const int lb : {3, 4})
            each_seq(la, [&](const std::vector<int>& a) {
                each_seq(lb, [&](const std::vector<int>& b) { check_merge(a, b); });
            });
    printf("checked=%ld bad=%ld\n", checked, bad);
    return bad ? 1 : 0;
}
