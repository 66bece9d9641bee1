// Host check of csrc/settle.h, the candidate sets of the rows the fused
// refinement settles itself, exhaustively over the 256 positions:
//  - settle_centroid maps the 2 x 8 x 16 (lane half, tile, score) positions one
//    to one onto centroids 0..255, in the MFMA D layout the kernel's winner
//    index uses (32 t + 8 (i / 4) + 4 h + i % 4);
//  - one marked score gives a set with exactly its centroid's bit, for every K
//    that keeps it and none for a K that drops it;
//  - the set of several marks is the union, the count the number of centroids
//    below K, and kth_candidate returns them in increasing order and -1 past
//    the last: all 256 marked, prefixes and strides, random subsets.
// Prints "bad=0" and exits 0 when all hold.
#include <cstdio>
#include <cstdint>
#include <set>
#include <vector>

#include "../crypto-recommendation_amd/csrc/settle.h"

using namespace lshkm;

static long bad = 0, checked = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        checked++;                                                      \
        if (!(c)) {                                                     \
            if (bad++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
        }                                                               \
    } while (0)

struct Pos { int h, t, i; };

// the set of the marked positions below K, through the kernel's own steps
static void check_set(const std::vector<Pos>& marks, int K) {
    LaneMask m[2] = {{0ull, 0ull}, {0ull, 0ull}};
    // a lane marks a tile at a time: gather each (half, tile)'s 16 flags first
    uint32_t bits[2][ST_TILES] = {};
    std::set<int> want;
    for (const Pos& p : marks) {
        bits[p.h][p.t] |= 1u << p.i;
        const int c = settle_centroid(p.h, p.t, p.i);
        if (c < K) want.insert(c);
    }
    for (int h = 0; h < 2; h++)
        for (int t = 0; t < ST_TILES; t++) settle_mark(m[h], t, bits[h][t]);
    unsigned long long cm[ST_CHUNKS];
    const int n = settle_set(m[0], m[1], K, cm);
    CHECK(n == (int)want.size());
    for (int c = 0; c < 64 * ST_CHUNKS; c++) CHECK((int)((cm[c >> 6] >> (c & 63)) & 1ull) == (int)want.count(c));
    int k = 0;
    for (const int c : want) CHECK(kth_candidate(cm, k++) == c);
    CHECK(kth_candidate(cm, k) == -1);
    CHECK(kth_candidate(cm, 255) == (n == 256 ? 255 : -1));
}

int main() {
    std::vector<Pos> all;
    std::set<int> seen;
    for (int h = 0; h < 2; h++)
        for (int t = 0; t < ST_TILES; t++)
            for (int i = 0; i < 16; i++) {
                const int c = settle_centroid(h, t, i);
                CHECK(c >= 0 && c < 256 && c / 32 == t && (c % 8) / 4 == h && c % 4 == i % 4 && (c % 32) / 8 == i / 4);
                seen.insert(c);
                all.push_back({h, t, i});
            }
    CHECK(seen.size() == 256);
    // one mark: its own bit alone, kept exactly by the K above its centroid
    for (const Pos& p : all) {
        const int c = settle_centroid(p.h, p.t, p.i);
        for (const int K : {1, c, c + 1, 63, 64, 65, 200, 256}) check_set({p}, K);
    }
    // all 256, and every K: the chunk edges among them
    for (int K = 1; K <= 256; K++) check_set(all, K);
    // prefixes in centroid order (3, 4, 64, 65 candidates) and strides
    std::vector<Pos> by_c(256);
    for (const Pos& p : all) by_c[settle_centroid(p.h, p.t, p.i)] = p;
    for (const int n : {1, 2, 3, 4, 63, 64, 65, 128, 255})
        for (const int first : {0, 1, 60, 100, 191}) {
            std::vector<Pos> v;
            for (int c = first; c < first + n && c < 256; c++) v.push_back(by_c[c]);
            for (const int K : {100, 250, 256}) check_set(v, K);
        }
    for (const int step : {2, 3, 4, 5, 8, 31, 32, 33, 64}) {
        std::vector<Pos> v;
        for (int c = step - 1; c < 256; c += step) v.push_back(by_c[c]);
        check_set(v, 256);
        check_set(v, 130);
    }
    // random subsets
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int rep = 0; rep < 400; rep++) {
        std::vector<Pos> v;
        for (int c = 0; c < 256; c++) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            if ((s >> 33) % 100 < (uint64_t)(rep % 50) * 2 + 1) v.push_back(by_c[c]);
        }
        check_set(v, 1 + (int)((s >> 40) % 256));
    }
    printf("checked=%ld bad=%ld\n", checked, bad);
    return bad ? 1 : 0;
}
