// gen_nearest_golden.cpp — golden fixtures of lshkm_min_vector_dist from the
// reference's own min_vector_euclidean_dist / min_vector_cosine_dist
// (lib/utils.hpp:107-140).
//
// Development-machine tool, not part of build(): it includes the reference's
// headers by path and needs its two translation units.
//
// (REF: the reference checkout, as in oracle/Makefile; the binary goes outside
// the repository):
//
//   g++ -std=c++11 -O0 -w -I$REF/lib -o $OUT/gen_nearest_golden tools/gen_nearest_golden.cpp \
//       $REF/lib/utils.cpp $REF/lib/data_structures/tweet.cpp
//   $OUT/gen_nearest_golden tests/golden/nearest
//
// A fixture <case>.npz holds data only:
//   x [N][d] f64 (the rows), q [nq][d] f64 (the queries), metric [1] i32
//   (0 euclidean, 1 cosine), f32 [1] i32 (1: every value is fp32-representable),
//   dist [nq] f64 (the helper's return value for query q over the vector of all
//   rows; also printed, as hex bits).
// The files are stored (uncompressed) zips with zeroed timestamps, so a rerun
// reproduces them byte for byte.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "utils.hpp"

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
static double unit() { return ((double)rnd() + 0.5) / 4294967296.0; }            // (0, 1)

enum Kind {
    GENERAL,     // general doubles: sums of s = x / sqrt(x^2 + 15) over x = k / 4 (crypto_rec.hpp:78-140's shape)
    F32,         // fp32-representable values, full mantissas
    DYADIC,      // multiples of 1/2 in [-2, 2]: many exact ties
    DUP,         // every odd row repeats the row before it
    ZERO0,       // GENERAL with a zero row at index 0
    ZERO_MID,    // ... at index N / 2 (and a zero query)
    INF0,        // GENERAL with an inf entry in row 0 (and a query with an inf in the same coordinate)
    INF_MID,     // ... in row N / 2
    BIG,         // GENERAL with 1e200 and 1e-200 entries in some rows and queries, and one all-1e-200 row
};

static double value(Kind k) {
    if (k == F32) return (double)(float)((unit() - 0.5) * 8.0);
    if (k == DYADIC) return (double)((int)(rnd() % 9) - 4) * 0.5;
    double v = 0.0;
    const int terms = 1 + rnd() % 3;
    for (int t = 0; t < terms; t++) {
        const double lex = (double)((int)(rnd() % 17) - 8) / 4.0 + (double)(rnd() % 3) * 0.25;
        v += lex / sqrt(lex * lex + 15.0);
    }
    return v;
}

struct Case {
    const char* name;
    Kind kind;
    int N, d, nq;
};

static bool run_case(const Case& cs, int metric, const std::string& dir) {
    g_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)(cs.N * 131 + cs.d * 7 + cs.nq);
    for (const char* p = cs.name; *p; p++) g_state = g_state * 31 + (unsigned char)*p;
    const int N = cs.N, d = cs.d, nq = cs.nq;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> x((size_t)N * d), q((size_t)nq * d);
    for (int i = 0; i < N; i++)
        for (int j = 0; j < d; j++)
            x[(size_t)i * d + j] = (cs.kind == DUP && (i & 1)) ? x[(size_t)(i - 1) * d + j] : value(cs.kind);
    // queries: every other one a row moved a little (or not at all), the rest fresh
    for (int i = 0; i < nq; i++)
        for (int j = 0; j < d; j++) {
            double v = value(cs.kind);
            if (N > 0 && (i & 1) == 0) {
                const double base = x[(size_t)((i * 37) % N) * d + j];
                v = (cs.kind == DYADIC || cs.kind == DUP || i % 4 == 0) ? base : base + v / 64.0;
                if (cs.kind == F32) v = (double)(float)v;
            }
            q[(size_t)i * d + j] = v;
        }
    if (N > 0) {
        const int mid = N / 2;
        if (cs.kind == ZERO0 || cs.kind == ZERO_MID)
            for (int j = 0; j < d; j++) x[(size_t)(cs.kind == ZERO0 ? 0 : mid) * d + j] = 0.0;
        if (cs.kind == ZERO_MID)
            for (int j = 0; j < d; j++) q[(size_t)(nq - 1) * d + j] = 0.0;
        if (cs.kind == INF0 || cs.kind == INF_MID) {
            x[(size_t)(cs.kind == INF0 ? 0 : mid) * d + 2] = inf;
            q[(size_t)(nq - 1) * d + 2] = inf;
            q[(size_t)(nq - 2) * d + 1] = -inf;
        }
        if (cs.kind == BIG) {
            x[(size_t)3 * d + 1] = 1e200;
            x[(size_t)(mid + 1) * d + 0] = -1e200;
            x[(size_t)5 * d + 2] = 1e-200;
            x[(size_t)(N - 1) * d + 3] = -1e-200;
            for (int j = 0; j < d; j++) x[(size_t)mid * d + j] = 1e-200;
            q[(size_t)(nq - 1) * d + 1] = 1e200;
            q[(size_t)(nq - 2) * d + 0] = 1e-200;
            for (int j = 0; j < d; j++) q[(size_t)(nq - 3) * d + j] = (j & 1) ? 1e-200 : -1e-200;
        }
    }
    std::vector<Vec> rows;
    rows.reserve(N);
    for (int i = 0; i < N; i++)
        rows.emplace_back("v" + std::to_string(i), std::vector<double>(x.begin() + (size_t)i * d, x.begin() + (size_t)(i + 1) * d));
    std::vector<double> dist(nq);
    const std::string name = std::string(metric ? "cos_" : "eu_") + cs.name;
    for (int i = 0; i < nq; i++) {
        Vec query("q" + std::to_string(i), std::vector<double>(q.begin() + (size_t)i * d, q.begin() + (size_t)(i + 1) * d));
        dist[i] = metric ? min_vector_cosine_dist<double, double>(&query, &rows)
                         : min_vector_euclidean_dist<double, double>(&query, &rows);
        uint64_t b;
        memcpy(&b, &dist[i], 8);
        printf("%s query %d dist %.17g bits 0x%016llx\n", name.c_str(), i, dist[i], (unsigned long long)b);
    }
    Npz z;
    z.f64("x", x, {(size_t)N, (size_t)d});
    z.f64("q", q, {(size_t)nq, (size_t)d});
    z.i32("metric", {metric});
    z.i32("f32", {cs.kind == F32 || cs.kind == DYADIC ? 1 : 0});
    z.f64("dist", dist, {(size_t)nq});
    return z.write(dir + "/" + name + ".npz");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <output directory>\n", argv[0]);
        return 2;
    }
    const Case cases[] = {
        {"general", GENERAL, 200, 17, 16}, {"f32", F32, 40, 128, 8},        {"dyadic", DYADIC, 600, 3, 64},
        {"dup", DUP, 200, 8, 16},          {"zero0", ZERO0, 100, 8, 8},     {"zero_mid", ZERO_MID, 100, 8, 8},
        {"inf0", INF0, 100, 8, 8},         {"inf_mid", INF_MID, 100, 8, 8}, {"big", BIG, 100, 8, 8},
        {"n1", GENERAL, 1, 17, 8},         {"n0", GENERAL, 0, 17, 4},
    };
    for (const Case& c : cases)
        for (int metric = 0; metric < 2; metric++)
            if (!run_case(c, metric, argv[1])) {
                fprintf(stderr, "cannot write %s\n", c.name);
                return 1;
            }
    return 0;
}
