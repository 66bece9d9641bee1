// Host check of lshkm_cube_p_closest's part of csrc/lshpc_layout.h
// (tests/test_cubepc_layout_cpu.py): the cube route's edges, and the screen's
// candidacy test (cubepc_probe + cubepc_member) against probe_masks enumerated
// literally, for every y of the cube.
#include <cstdio>

#include "../crypto-recommendation_amd/csrc/lshpc_layout.h"

using namespace lshkm;

static long bad = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) { bad++; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

int main() {
    // the rule: d <= 128, k <= 30, P + 1 + 64 <= 512, whatever the metric
    CHECK(cubepc_route(100, 6, 20, false) == LshpcRoute::screen);
    CHECK(cubepc_route(1, 1, 1, false) == LshpcRoute::screen);
    CHECK(cubepc_route(128, 30, 447, false) == LshpcRoute::screen);
    CHECK(cubepc_route(128, 30, 448, false) == LshpcRoute::lists);
    CHECK(cubepc_route(129, 6, 20, false) == LshpcRoute::lists);
    CHECK(cubepc_route(100, 31, 20, false) == LshpcRoute::lists);
    CHECK(cubepc_route(100, 6, 20, true) == LshpcRoute::lists);
    CHECK(cubepc_route(100, 6, 2147483647, false) == LshpcRoute::lists);

    CHECK(cubepc_rev(1u) == 0x80000000u && cubepc_rev(0x80000000u) == 1u && cubepc_rev(6u) == 0x60000000u);
    CHECK(cubepc_choose(30, 15) == 155117520 && cubepc_choose(5, 0) == 1 && cubepc_choose(5, 6) == 0);

    long sets = 0;
    for (int k = 1; k <= 16; k++) {
        const int all = 1 << k;
        const int probes_of[] = {-1, 0, 1, 2, 3, k - 1, k, k + 1, k + 2, k * (k - 1) / 2 + k - 1, k * (k - 1) / 2 + k,
                                 k * (k - 1) / 2 + k + 1, all - 2, all - 1, all, all + 1, 2147483647};
        for (int probes : probes_of) {
            const std::vector<int32_t> masks = probe_masks(probes, k);
            std::vector<char> in((size_t)all, 0);
            for (int32_t m : masks) {
                CHECK(m >= 0 && m < all && !in[(size_t)m]);         // the list names every bucket once
                in[(size_t)m] = 1;
            }
            const CubeProbe pr = cubepc_probe(probes, k);
            long differ = 0, members = 0;
            for (int y = 0; y < all; y++) {
                const bool got = cubepc_member((uint32_t)y, pr.shells, pr.rev_last);
                differ += got != (in[(size_t)y] != 0);
                members += got;
            }
            if (differ) std::printf("k=%d probes=%d: %ld of %d differ\n", k, probes, differ, all);
            CHECK(differ == 0);
            CHECK(members == (long)masks.size());
            sets++;
        }
        // the named cases
        CHECK(probe_masks(0, k).size() == 1);                                       // the main bucket only
        CHECK(probe_masks(1, k).size() == (k >= 2 ? 2u : 1u));                      // the quirk: no distance-1 mask
        if (k >= 2) CHECK(probe_masks(1, k)[1] == 3);
        CHECK((int)probe_masks(all, k).size() == (k >= 1 ? all : 1));               // beyond the cube: every row
    }
    // every probes of two small cubes, so that every prefix length of every shell is met
    for (int k : {5, 7})
        for (int probes = 0; probes <= (1 << k) + 1; probes++) {
            const std::vector<int32_t> masks = probe_masks(probes, k);
            std::vector<char> in((size_t)1 << k, 0);
            for (int32_t m : masks) in[(size_t)m] = 1;
            const CubeProbe pr = cubepc_probe(probes, k);
            for (int y = 0; y < (1 << k); y++)
                CHECK(cubepc_member((uint32_t)y, pr.shells, pr.rev_last) == (in[(size_t)y] != 0));
            sets++;
        }
    // a wide cube: the boundary mask of a partial shell, without enumerating 2^30 vertices
    {
        const int k = 30, probes = 30 + 100;                   // distance 1 whole, 100 masks of distance 2
        const std::vector<int32_t> masks = probe_masks(probes, k);
        const CubeProbe pr = cubepc_probe(probes, k);
        for (int32_t m : masks) CHECK(cubepc_member((uint32_t)m, pr.shells, pr.rev_last));
        long members2 = 0;
        for (int i = 0; i < k; i++)
            for (int j = i + 1; j < k; j++) members2 += cubepc_member(1u << i | 1u << j, pr.shells, pr.rev_last);
        CHECK(members2 == 100);
        CHECK(!cubepc_member(7u, pr.shells, pr.rev_last));
    }
    std::printf("sets=%ld bad=%ld\n", sets, bad);
    return bad ? 1 : 0;
}
