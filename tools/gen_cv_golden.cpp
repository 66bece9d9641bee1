// gen_cv_golden.cpp — golden fixtures of the recommender's 10-fold validation
// from the reference's own functions: split_to_10, merge_except_for,
// hide_one_score, get_P_closest, get_predicted_user_sim (lib/crypto_rec.hpp),
// create_LSH_hashtables, get_LSH_filtered_combined_buckets (lib/lsh_cube.hpp)
// and lsh_rec_10_fold_validation_A (main.cpp:393-437).
//
// Development-machine tool, not part of build(): it includes the reference's
// sources by path (REF: the reference checkout, as in oracle/Makefile; the
// binary goes outside the repository):
//
//   g++ -std=c++11 -O0 -w -I$REF -I$REF/lib -o $OUT/gen_cv_golden tools/gen_cv_golden.cpp \
//       $REF/lib/utils.cpp $REF/lib/data_structures/tweet.cpp $REF/lib/in_out/arg_parser.cpp
//   $OUT/gen_cv_golden tests/golden/cv
//   $OUT/gen_cv_golden --time 20000      (the baseline: seconds of the reference's function)
//
// The fold loop. Both: main.cpp is included with `main` renamed by a macro and
// its lsh_rec_10_fold_validation_A gives the stored result; the loop of
// main.cpp:399-433 is also written out below, calling the same functions, to
// record what the function keeps to itself (per-user hide results, neighbour
// counts and errors, per-fold sums). The tool fails unless both agree bit for
// bit.
//
// Determinism: time() is interposed with a constant (split_to_10's and
// hide_one_score's srand((int)time(0))), std::chrono::_V2::system_clock::now()
// with a counter (create_LSH_hashtables' seed, one read per fold), as the
// oracle harness does. Both are recorded as the seeds. std::cout is silenced.
//
// A fixture <case>.npz holds data only (M = 10 * (N / 10), F = N / 10):
//   x [N][d] f64, x_mean [N] f64, unk_ptr [N+1] i64, unk_idx i32: the users;
//   params [7] i32: metric (0 euclidean, 1 cosine), k, L, lsh_bucket_div, P, N, d;
//   w [1] f64; split_seed / hide_seed [1] i64 (the time() constant), lsh_seeds [10] i64;
//   split [10*F] i32: user indexes in fold order;
//   per user in split order: hide_ret [M] i32 (hide_one_score's return value),
//   hide_idx [M] i32 (-1 where false), old_score [M] f64, h [M][d] f64,
//   h_mean [M] f64 (the user after the call), nb_cnt [M] i32 (the filtered
//   union's size; -1: not queried), err [M] f64 (fabs(old_score - prediction);
//   -1.0: skipped);
//   fold_sum [10] f64 (k_sum), fold_cnt [10] i32 (calc_user_num), mae [1] f64.
// The files are stored (uncompressed) zips with zeroed timestamps, so a rerun
// reproduces them byte for byte.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <set>
#include <string>
#include <vector>

static long long g_clock = 0;       // the next system_clock::now() reading
static const long g_time = 1546300800;   // time(0): 2019-01-01 00:00:00 UTC

namespace std { namespace chrono { inline namespace _V2 {
system_clock::time_point system_clock::now() noexcept {
    return system_clock::time_point(system_clock::duration(g_clock++));
}
}}}

extern "C" time_t time(time_t* t) noexcept {
    if (t) *t = (time_t)g_time;
    return (time_t)g_time;
}

#define main reference_main
#include "main.cpp"
#undef main

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
    void f64(const std::string& n, const std::vector<double>& v) { add(n, "<f8", {v.size()}, v.data(), v.size() * 8); }
    void i32(const std::string& n, const std::vector<int32_t>& v) { add(n, "<i4", {v.size()}, v.data(), v.size() * 4); }
    void i64(const std::string& n, const std::vector<int64_t>& v) { add(n, "<i8", {v.size()}, v.data(), v.size() * 8); }
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
// Counter-based values (splitmix64 of seed + index), so the benchmark's row
// (tools/bench_rows.py, "cv") forms the same users without a file.
static uint64_t mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// a score in [-1, 3): a 53-bit fraction, so general doubles
static double score_at(uint64_t seed, uint64_t idx) { return (double)(mix(seed + 2 * idx) >> 11) * (1.0 / 9007199254740992.0) * 4.0 - 1.0; }
// known with probability known_256 / 256
static bool known_at(uint64_t seed, uint64_t idx, int known_256) { return (int)(mix(seed + 2 * idx + 1) >> 56) < known_256; }

struct User {
    std::vector<double> dims;
    std::set<int> unk;
    double mean;
};

// Shaped like tweets_to_user_vectors (crypto_rec.hpp:105-137): known scores,
// the mean = their sum in index order / their number, unknown indexes holding it.
static User shaped(const std::vector<double>& score, const std::vector<bool>& known) {
    User u;
    const int d = (int)score.size();
    double sum = 0;
    int n = 0;
    for (int j = 0; j < d; j++)
        if (known[j]) { sum = sum + score[j]; n++; } else u.unk.emplace(j);
    u.mean = n ? sum / n : 0.5;      // no known index: an arbitrary mean (the reference never builds such a user)
    u.dims = score;
    for (int j : u.unk) u.dims[j] = u.mean;
    return u;
}

static User plain_user(uint64_t seed, int i, int d, int known_256) {
    std::vector<double> s(d);
    std::vector<bool> kn(d);
    int n = 0;
    for (int j = 0; j < d; j++) {
        s[j] = score_at(seed, (uint64_t)i * d + j);
        kn[j] = known_at(seed, (uint64_t)i * d + j, known_256);
        n += kn[j];
    }
    for (int j = 0; n < 2 && j < d; j++)         // at least two known scores
        if (!kn[j]) { kn[j] = true; n++; }
    return shaped(s, kn);
}

struct Case {
    const char* name;
    const char* metric;
    int N, d, k, L, div, P;
    double w;
    int known_256;
    int kind;          // 0 plain, 1 sparse, 2 nan
};

struct Result {
    std::vector<int32_t> split, hide_ret, hide_idx, nb_cnt, fold_cnt;
    std::vector<double> old_score, h, h_mean, err, fold_sum;
    double mae;
    int n_empty, n_nonempty, n_lt2, n_useless, n_on_unknown;
};

// main.cpp:393-437 written out, calling the reference's functions, recording as it goes
static Result run_loop(std::vector<Vec>& users, const std::vector<User>& src, const Case& cs) {
    Result r;
    r.n_empty = r.n_nonempty = r.n_lt2 = r.n_useless = r.n_on_unknown = 0;
    const int d = cs.d;
    std::vector<std::vector<Vec> > separate_vectors = split_to_10<double>(users);
    for (auto& fold : separate_vectors)
        for (auto& u : fold) r.split.push_back(atoi(u.getId().c_str() + 1));
    double all_sum = 0;
    for (int i = 0; i < 10; i++) {
        double k_sum = 0;
        std::vector<Vec> curr_known = merge_except_for<double>(separate_vectors, i);
        std::vector<CustHashtable<double>*> tabs =
            create_LSH_hashtables<double>(curr_known, cs.metric, cs.k, cs.L, cs.div, cs.w);
        int calc_user_num = 0;
        for (auto& user : separate_vectors[i]) {
            const User& before = src[atoi(user.getId().c_str() + 1)];
            double old_score = 0;
            const bool calculate = hide_one_score(user, &old_score);
            int nb = -1;
            double err = -1.0;
            if (calculate) {
                std::vector<Vec*> neighbors = get_LSH_filtered_combined_buckets(tabs, &user);
                nb = (int)neighbors.size();
                if (!neighbors.empty()) {
                    r.n_nonempty++;
                    std::vector<double> similarities = get_P_closest(neighbors, user, cs.P);
                    std::vector<double> pred = get_predicted_user_sim(neighbors, user, similarities);
                    const int new_index = user.getUnknownIndexes().at(0);
                    err = fabs(old_score - pred[new_index]);
                    k_sum = k_sum + err;
                    calc_user_num++;
                } else {
                    r.n_empty++;
                }
            } else if (d - (int)before.unk.size() < 2) {
                r.n_lt2++;
            } else {
                r.n_useless++;
            }
            const int hidx = calculate ? user.getUnknownIndexes().at(0) : -1;
            if (calculate && before.unk.count(hidx)) r.n_on_unknown++;
            r.hide_ret.push_back(calculate);
            r.hide_idx.push_back(hidx);
            r.old_score.push_back(old_score);
            for (int j = 0; j < d; j++) r.h.push_back(user.getDimensions()->at(j));
            r.h_mean.push_back(user.getKnownMean());
            r.nb_cnt.push_back(nb);
            r.err.push_back(err);
        }
        if (calc_user_num > 0) all_sum = all_sum + (k_sum / calc_user_num);
        r.fold_sum.push_back(k_sum);
        r.fold_cnt.push_back(calc_user_num);
        for (size_t t = 0; t < tabs.size(); t++) delete tabs[t];
    }
    r.mae = all_sum / 10;
    return r;
}

static std::vector<User> make_users(const Case& cs, uint64_t seed) {
    std::vector<User> us;
    srand((int)time(0));
    const int draw = rand();                      // hide_one_score's rand() under the constant time()
    for (int i = 0; i < cs.N; i++) {
        User u = plain_user(seed, i, cs.d, cs.known_256);
        const int d = cs.d;
        if (cs.kind == 1) {
            std::vector<double> s(d);
            std::vector<bool> kn(d, false);
            for (int j = 0; j < d; j++) s[j] = score_at(seed, (uint64_t)i * d + j);
            switch (i % 8) {
                case 1: u = shaped(s, kn); break;                                  // no known index: false, unchanged
                case 3: kn[i % d] = true; u = shaped(s, kn); break;               // one known index: false, unchanged
                case 5: {                                                         // "useless": zeroed, not calculated
                    kn[0] = kn[1] = true;                                         // hide_index = draw % 2 is known
                    s[draw % 2] = 0.75;
                    s[1 - draw % 2] = 0.0;
                    u = shaped(s, kn);
                    break;
                }
                case 7: kn[d - 1] = kn[d - 2] = kn[d - 3] = true; u = shaped(s, kn); break;   // draw % 3 < d - 3: unknown
                default: break;
            }
        }
        if (cs.kind == 2 && i % 9 == 4) {                                         // a zero row: NaN similarities
            std::vector<double> s(d, 0.0);
            std::vector<bool> kn(d, false);
            kn[0] = kn[2] = true;
            u = shaped(s, kn);
        }
        us.push_back(u);
    }
    return us;
}

static std::vector<Vec> to_vecs(const std::vector<User>& us) {
    std::vector<Vec> v;
    v.reserve(us.size());
    for (size_t i = 0; i < us.size(); i++) v.emplace_back("u" + std::to_string(i), us[i].dims, us[i].unk, us[i].mean);
    return v;
}

static uint64_t bits(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

static bool run_case(const Case& cs, const std::string& dir) {
    uint64_t seed = 0xC0FFEEull;
    for (const char* p = cs.name; *p; p++) seed = seed * 131 + (unsigned char)*p;
    const std::vector<User> us = make_users(cs, seed);
    const long long clock0 = 1000 * (long long)(seed % 1000) + 7;

    std::vector<Vec> a = to_vecs(us);
    g_clock = clock0;
    const double own = lsh_rec_10_fold_validation_A(a, cs.metric, cs.k, cs.L, cs.div, cs.w, cs.P);   // main.cpp's
    std::vector<Vec> b = to_vecs(us);
    g_clock = clock0;
    const Result r = run_loop(b, us, cs);
    if (bits(own) != bits(r.mae)) {
        fprintf(stderr, "%s: main.cpp's function gives %016llx, the written-out loop %016llx\n", cs.name,
                (unsigned long long)bits(own), (unsigned long long)bits(r.mae));
        return false;
    }
    int folds = 0;
    for (int c : r.fold_cnt) folds += c > 0;
    fprintf(stderr, "%s: mae %.17g (%016llx), folds with users %d, empty %d, non-empty %d, <2 %d, useless %d, on-unknown %d\n",
            cs.name, r.mae, (unsigned long long)bits(r.mae), folds, r.n_empty, r.n_nonempty, r.n_lt2, r.n_useless,
            r.n_on_unknown);
    if (cs.kind != 2 && folds < 8) { fprintf(stderr, "%s: fewer than 8 folds with users\n", cs.name); return false; }
    if (cs.kind == 2 && r.mae == r.mae) { fprintf(stderr, "%s: the result is not NaN\n", cs.name); return false; }
    if (cs.kind == 1 && !(r.n_lt2 >= 2 && r.n_useless >= 1 && r.n_on_unknown >= 1)) {
        fprintf(stderr, "%s: a branch of hide_one_score does not occur\n", cs.name);
        return false;
    }
    if (!strcmp(cs.metric, "euclidean") && !(r.n_empty >= 1 && r.n_nonempty >= 1)) {
        fprintf(stderr, "%s: needs both empty and non-empty filtered unions\n", cs.name);
        return false;
    }

    const int N = cs.N, d = cs.d;
    std::vector<double> x, xm;
    std::vector<int64_t> up(1, 0);
    std::vector<int32_t> ui;
    for (const User& u : us) {
        x.insert(x.end(), u.dims.begin(), u.dims.end());
        xm.push_back(u.mean);
        for (int j : u.unk) ui.push_back(j);
        up.push_back((int64_t)ui.size());
    }
    std::vector<int64_t> lsh_seeds;
    for (int i = 0; i < 10; i++) lsh_seeds.push_back(clock0 + i);
    Npz z;
    z.f64("x", x, {(size_t)N, (size_t)d});
    z.f64("x_mean", xm);
    z.i64("unk_ptr", up);
    z.i32("unk_idx", ui);
    z.i32("params", {strcmp(cs.metric, "euclidean") ? 1 : 0, cs.k, cs.L, cs.div, cs.P, N, d});
    z.f64("w", {cs.w});
    z.i64("split_seed", {(int64_t)g_time});
    z.i64("hide_seed", {(int64_t)g_time});
    z.i64("lsh_seeds", lsh_seeds);
    z.i32("split", r.split);
    z.i32("hide_ret", r.hide_ret);
    z.i32("hide_idx", r.hide_idx);
    z.f64("old_score", r.old_score);
    z.f64("h", r.h, {r.h_mean.size(), (size_t)d});
    z.f64("h_mean", r.h_mean);
    z.i32("nb_cnt", r.nb_cnt);
    z.f64("err", r.err);
    z.f64("fold_sum", r.fold_sum);
    z.i32("fold_cnt", r.fold_cnt);
    z.f64("mae", {r.mae});
    return z.write(dir + "/" + cs.name + ".npz");
}

// The baseline: the reference's own function on the benchmark row's users
// (tools/bench_rows.py "cv": cosine, d = 100, k = 4, L = 5, P = 20).
static int time_reference(int N) {
    const Case cs = {"time", "cosine", N, 100, 4, 5, 4, 20, 0.01, 128, 0};
    const std::vector<User> us = make_users(cs, 0xBE7C4ull);
    std::vector<Vec> a = to_vecs(us);
    g_clock = 1;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    const double mae = lsh_rec_10_fold_validation_A(a, cs.metric, cs.k, cs.L, cs.div, cs.w, cs.P);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    printf("{\"row\": \"cv_reference\", \"N\": %d, \"d\": 100, \"k\": 4, \"L\": 5, \"P\": 20, \"seconds\": %.3f, \"mae\": %.17g}\n",
           N, (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec), mae);
    return 0;
}

int main(int argc, char** argv) {
    std::cout.setstate(std::ios_base::failbit);      // the reference's progress lines
    if (argc == 3 && !strcmp(argv[1], "--time")) return time_reference(atoi(argv[2]));
    if (argc != 2) {
        fprintf(stderr, "usage: %s <output directory> | --time <N>\n", argv[0]);
        return 2;
    }
    const Case cases[] = {
        {"cos", "cosine", 203, 12, 3, 3, 4, 5, 0.01, 160, 0},
        {"cos_bigp", "cosine", 100, 12, 3, 3, 4, 1000, 0.01, 160, 0},
        {"eu", "euclidean", 200, 8, 2, 3, 4, 5, 0.5, 160, 0},
        {"sparse", "cosine", 160, 10, 2, 3, 4, 4, 0.01, 160, 1},
        {"nan", "cosine", 100, 8, 2, 2, 4, 6, 0.01, 160, 2},
    };
    for (const Case& c : cases)
        if (!run_case(c, argv[1])) {
            fprintf(stderr, "cannot produce %s\n", c.name);
            return 1;
        }
    return 0;
}
