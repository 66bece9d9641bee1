// gen_pam_golden.cpp — golden fixtures of the PAM medoid update from the
// reference's own pam_lloyds (lib/clustering_phases/update.hpp:89-142).
//
// Development-machine tool, not part of build(): it includes the reference's
// headers by path and needs its two translation units.
//
// (REF: the reference checkout, as in oracle/Makefile; the binary goes outside
// the repository):
//
//   g++ -std=c++11 -O0 -w -I$REF/lib -o $OUT/gen_pam_golden tools/gen_pam_golden.cpp \
//       $REF/lib/utils.cpp $REF/lib/data_structures/tweet.cpp
//   $OUT/gen_pam_golden tests/golden/pam
//
// Every case runs pam_lloyds twice on one assignment: from the stored previous
// centroids, then from its own result (which must not swap again). A fixture
// <case>.npz holds data only:
//   x [N][d] f64, assign [N] i32, metric [1] i32 (0 euclidean, 1 cosine),
//   prev_rows [K] i32 (-1: a "k_means_center"), medoid_rows / medoid_rows2 [K]
//   i32, swapped / swapped2 [1] i32, sums / sums2 [K] f64 (each cluster's
//   winning dist_sum, accumulated as the reference does: cached reverse pairs
//   for j < p; also printed, as hex bits).
// The files are stored (uncompressed) zips with zeroed timestamps, so a rerun
// reproduces them byte for byte.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "utils.hpp"
#include "clustering_phases/update.hpp"

typedef CustVector<double> Vec;

// ------------------------------------------------------------- npz (stored)
static uint32_t crc32_of(const std::string& s) {
    static uint32_t tab[256];
    static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            tab[i] = c;
        }
        init = true;
    }
    uint32_t c = 0xFFFFFFFFu;
    for (unsigned char ch : s) c = tab[(c ^ ch) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

static void put(std::string& o, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; i++) o.push_back((char)((v >> (8 * i)) & 0xFF));
}

struct Npz {
    struct Entry { std::string name, data; };
    std::vector<Entry> entries;
    void add(const std::string& name, const char* descr, const std::vector<size_t>& shape, const void* p, size_t bytes) {
        std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (";
        for (size_t i = 0; i < shape.size(); i++) dict += std::to_string(shape[i]) + (shape.size() == 1 || i + 1 < shape.size() ? "," : "");
        dict += "), }";
        while ((10 + dict.size() + 1) % 64) dict.push_back(' ');
        dict.push_back('\n');
        std::string d("\x93NUMPY\x01\x00", 8);
        put(d, dict.size(), 2);
        d += dict;
        d.append((const char*)p, bytes);
        entries.push_back({name + ".npy", d});
    }
    void f64(const std::string& n, const std::vector<double>& v, std::vector<size_t> shape) { add(n, "<f8", shape, v.data(), v.size() * 8); }
    void i32(const std::string& n, const std::vector<int32_t>& v) { add(n, "<i4", {v.size()}, v.data(), v.size() * 4); }
    bool write(const std::string& path) const {
        std::string out, central;
        for (const Entry& e : entries) {
            const uint32_t crc = crc32_of(e.data), off = (uint32_t)out.size();
            std::string h;
            put(h, 0x04034b50, 4); put(h, 20, 2); put(h, 0, 2); put(h, 0, 2); put(h, 0, 2); put(h, 0x21, 2);
            put(h, crc, 4); put(h, e.data.size(), 4); put(h, e.data.size(), 4); put(h, e.name.size(), 2); put(h, 0, 2);
            out += h + e.name + e.data;
            std::string c;
            put(c, 0x02014b50, 4); put(c, 20, 2); put(c, 20, 2); put(c, 0, 2); put(c, 0, 2); put(c, 0, 2); put(c, 0x21, 2);
            put(c, crc, 4); put(c, e.data.size(), 4); put(c, e.data.size(), 4); put(c, e.name.size(), 2);
            put(c, 0, 2); put(c, 0, 2); put(c, 0, 2); put(c, 0, 2); put(c, 0, 4); put(c, off, 4);
            central += c + e.name;
        }
        const uint32_t coff = (uint32_t)out.size();
        out += central;
        put(out, 0x06054b50, 4); put(out, 0, 2); put(out, 0, 2); put(out, entries.size(), 2); put(out, entries.size(), 2);
        put(out, central.size(), 4); put(out, coff, 4); put(out, 0, 2);
        FILE* f = fopen(path.c_str(), "wb");
        if (!f) return false;
        const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
        fclose(f);
        return ok;
    }
};

// -------------------------------------------------------------------- inputs
static uint64_t g_state;
static uint32_t rnd() {   // a 64-bit LCG's high half
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

// multiples of 2^-15 around K planted centres
static double grid_value(int c, int j) {
    const double centre = (double)(((c * 37 + j * 11) % 17) - 8) * 0.25;
    return centre + ((double)(rnd() % 65536) - 32768.0) / 32768.0;
}

// general doubles shaped like tweets_to_user_vectors (crypto_rec.hpp:78-140):
// sums of sentiment scores s = x / sqrt(x^2 + 15) over lexicon sums x = k / 4
static double user_value(int c, int j) {
    double v = 0.0;
    const int terms = 1 + rnd() % 3;
    for (int t = 0; t < terms; t++) {
        const double lex = (double)((int)(rnd() % 17) - 8 + ((c + j) % 5)) / 4.0;
        v += lex / sqrt(lex * lex + 15.0);
    }
    return v;
}

struct Case {
    const char* name;
    const char* metric;
    int N, d, K;
    bool full;        // user_value rows (else grid)
    bool dup;         // every odd row repeats the row before it
    int zero_every;   // rows 0, z, 2z, ... are zero vectors where they fall in clusters 0 and 1
    bool kmc;         // previous centroids are "k_means_center" vectors
};

static double pair_dist(Vec* a, Vec* b, const std::string& metric) {
    return metric == "euclidean" ? a->euclideanDistance(b) : a->cosineDistance(b);
}

// dist_sum of member p as update.hpp:103-123 accumulates it: d(x_j, x_p) from
// the cache for j < p (stored by j's pass), d(x_p, x_j) computed for j >= p
static double dist_sum_of(std::vector<Vec*>& cl, size_t p, const std::string& metric) {
    double s = 0;
    for (size_t j = 0; j < cl.size(); j++) s = s + (j < p ? pair_dist(cl[j], cl[p], metric) : pair_dist(cl[p], cl[j], metric));
    return s;
}

static bool run_case(const Case& cs, const std::string& dir) {
    g_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)(cs.N * 131 + cs.d * 7 + cs.K);
    for (const char* p = cs.name; *p; p++) g_state = g_state * 31 + (unsigned char)*p;
    const std::string metric = cs.metric;
    std::vector<Vec> in;
    std::vector<double> x((size_t)cs.N * cs.d);
    std::vector<int32_t> assign(cs.N);
    in.reserve(cs.N);
    for (int i = 0; i < cs.N; i++) {
        const int c = (int)(rnd() % cs.K);
        assign[i] = i < cs.K ? i : c;                      // no empty cluster
        std::vector<double> dims(cs.d);
        for (int j = 0; j < cs.d; j++) dims[j] = cs.full ? user_value(assign[i], j) : grid_value(assign[i], j);
        if (cs.dup && (i & 1) && i >= cs.K + 1) {
            assign[i] = assign[i - 1];
            for (int j = 0; j < cs.d; j++) dims[j] = x[(size_t)(i - 1) * cs.d + j];
        }
        if (cs.zero_every && i % cs.zero_every == 0 && assign[i] < 2)   // clusters 2.. keep finite sums
            for (int j = 0; j < cs.d; j++) dims[j] = 0.0;
        for (int j = 0; j < cs.d; j++) x[(size_t)i * cs.d + j] = dims[j];
        in.emplace_back("v" + std::to_string(i), dims, assign[i], 0.0);
    }
    // previous centroids: a member of each cluster (the last one), or k_means_center vectors
    std::vector<Vec*> cent(cs.K);
    std::vector<int32_t> prev(cs.K, -1);
    std::vector<Vec*> owned;
    for (int c = 0; c < cs.K; c++) {
        if (cs.kmc) {
            cent[c] = new Vec("k_means_center", std::vector<double>(cs.d, 0.25 * c));
            owned.push_back(cent[c]);
            continue;
        }
        for (int i = 0; i < cs.N; i++)
            if (assign[i] == c) prev[c] = i;
        cent[c] = &in[prev[c]];
    }
    Npz z;
    z.f64("x", x, {(size_t)cs.N, (size_t)cs.d});
    z.i32("assign", assign);
    z.i32("metric", {metric == "euclidean" ? 0 : 1});
    z.i32("prev_rows", prev);
    for (int run = 0; run < 2; run++) {
        const bool swapped = pam_lloyds(in, cent, metric);
        std::vector<std::vector<Vec*> > clusters = separate_clusters_from_input(in, cs.K);
        std::vector<int32_t> med(cs.K);
        std::vector<double> sums(cs.K);
        for (int c = 0; c < cs.K; c++) {
            med[c] = (int32_t)(cent[c] - &in[0]);
            size_t p = 0;
            while (clusters[c][p] != cent[c]) p++;
            sums[c] = dist_sum_of(clusters[c], p, metric);
            uint64_t b;
            memcpy(&b, &sums[c], 8);
            printf("%s run %d cluster %d medoid row %d dist_sum %.17g bits 0x%016llx\n", cs.name, run, c, med[c], sums[c],
                   (unsigned long long)b);
        }
        printf("%s run %d swapped %d\n", cs.name, run, (int)swapped);
        const std::string sfx = run ? "2" : "";
        z.i32("medoid_rows" + sfx, med);
        z.i32("swapped" + sfx, {(int32_t)swapped});
        z.f64("sums" + sfx, sums, {(size_t)cs.K});
    }
    for (Vec* v : owned) delete v;
    return z.write(dir + "/" + cs.name + ".npz");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <output directory>\n", argv[0]);
        return 2;
    }
    const Case cases[] = {
        {"eu_grid", "euclidean", 600, 16, 6, false, false, 0, false},
        {"eu_full", "euclidean", 400, 100, 5, true, false, 0, false},
        {"cos_grid", "cosine", 500, 8, 4, false, false, 0, false},
        {"cos_full", "cosine", 300, 16, 3, true, false, 0, false},
        {"eu_dup", "euclidean", 300, 8, 3, false, true, 0, false},
        {"cos_zero", "cosine", 400, 16, 4, false, false, 37, false},
        {"eu_kmc", "euclidean", 300, 8, 12, false, false, 0, true},
        {"cos_full_kmc", "cosine", 240, 100, 3, true, false, 0, true},
    };
    for (const Case& c : cases)
        if (!run_case(c, argv[1])) {
            fprintf(stderr, "cannot write %s\n", c.name);
            return 1;
        }
    return 0;
}
