// Host probe of crypto-recommendation_amd/csrc/kmseg.h for one given chain:
// the segmented evaluation exactly as tests/kmseg_check.cpp models update.hip's
// passes (pairs = the chain cut at window boundaries, the first pair starting at
// a given window offset; A pair sums, B approximate pair starts, C records per
// pair, D composition), without perturbing the predictions. It reports which
// branches of the composition the chain takes: the record count of every pair,
// the summaries that did not apply (walked with real adds), the dense pairs
// (more than KS_R records), and whether the result equals the plain chain.
//
// Input file: little-endian fp64 values [start, window offset, x_0, x_1, ...].
// Output: one line
//   pairs=<n> counts=<c0,c1,...> fails=<n> dense=<n> equal=<0|1>
// Built and run by tests/test_update_edges_cpu.py (CPU).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../crypto-recommendation_amd/csrc/kmseg.h"

using namespace lshkm;

static volatile double g_sink;

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: kmseg_probe FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double v;
    while (fread(&v, 8, 1, f) == 1) in.push_back(v);
    fclose(f);
    if (in.size() < 2) { fprintf(stderr, "short file\n"); return 2; }
    const double s0 = in[0];
    const int off0 = (int)in[1];
    if (off0 < 0 || off0 >= KS_W) { fprintf(stderr, "bad offset\n"); return 2; }
    const std::vector<double> x(in.begin() + 2, in.end());
    const int n = (int)x.size();

    double want = s0;
    for (double xi : x) { want = want + xi; g_sink = want; }

    std::vector<int> pb;                      // pair starts
    for (int p = 0; p < n;) {
        pb.push_back(p);
        p += KS_W - (p == 0 ? off0 : 0);
    }
    pb.push_back(n);
    const int np = (int)pb.size() - 1;
    std::vector<double> psum(np), sin(np);
    for (int q = 0; q < np; q++) {            // A
        double t = 0.0;
        for (int p = pb[q]; p < std::min(pb[q + 1], n); p++) t += x[p];
        psum[q] = t;
    }
    double run = s0;                          // B
    for (int q = 0; q < np; q++) { sin[q] = run; run += psum[q]; }
    std::vector<std::vector<KsRec>> recs(np);
    std::vector<int> cnt(np);
    for (int q = 0; q < np; q++) {            // C
        const int beg = pb[q], end = std::min(pb[q + 1], n);
        const int obase = (q == 0) ? off0 : 0;
        double sa = sin[q];
        KsSeg g;
        bool open = false;
        int nr = 0;
        auto emit = [&](const KsSeg& gg) {
            if (nr < KS_R) recs[q].push_back(ks_record(gg));
            nr++;
        };
        for (int p = beg; p < end; p++) {
            sa += x[p];
            ks_feed(g, open, x[p], sa, obase + (p - beg), emit);
        }
        if (open) emit(g);
        cnt[q] = nr;
    }
    long fails = 0, dense = 0;
    double s = s0;                            // D
    for (int q = 0; q < np; q++) {
        const int beg = pb[q], end = std::min(pb[q + 1], n);
        const int obase = (q == 0) ? off0 : 0;
        if (cnt[q] > KS_R) {
            dense++;
            for (int p = beg; p < end; p++) { s = s + x[p]; g_sink = s; }
            continue;
        }
        for (const KsRec& r : recs[q]) {
            if (!ks_apply(s, r)) {
                fails++;
                for (int o = ks_rec_a(r) + 1; o <= ks_rec_b(r); o++) { s = s + x[beg + (o - obase)]; g_sink = s; }
            }
        }
    }
    const bool equal = memcmp(&s, &want, 8) == 0 || (std::isnan(s) && std::isnan(want));
    printf("pairs=%d counts=", np);
    for (int q = 0; q < np; q++) printf("%s%d", q ? "," : "", cnt[q]);
    printf(" fails=%ld dense=%ld equal=%d\n", fails, dense, equal ? 1 : 0);
    return equal ? 0 : 1;
}
