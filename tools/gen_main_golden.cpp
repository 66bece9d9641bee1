// gen_main_golden.cpp — golden fixtures of the whole program: the reference's
// own main (main.cpp:36-390) run on generated inputs, its output file and its
// standard output recorded.
//
// Development-machine tool, not part of build(): it includes the reference's
// sources by path (REF: the reference checkout, as in oracle/Makefile; the
// binary goes outside the repository):
//
//   g++ -std=c++11 -O0 -w -I$REF -I$REF/lib -o $OUT/gen_main_golden tools/gen_main_golden.cpp \
//       $REF/lib/utils.cpp $REF/lib/data_structures/tweet.cpp $REF/lib/in_out/arg_parser.cpp
//   $OUT/gen_main_golden tests/golden/main
//   $OUT/gen_main_golden --time FACTOR DIR   (the baseline: seconds of the reference's main on the
//                                             mid inputs with every count times FACTOR, written to DIR)
//
// main.cpp is included with `main` renamed by a macro; the tool changes into
// the case directory (the program reads ./cluster.conf and the configuration's
// relative paths) and calls it with -d <tweet file> -o expected.out, and with
// -validate where the case says so. Its return value is ignored: the
// reference's main ends without a return statement.
//
// Determinism: std::chrono::_V2::system_clock::now() is defined here as a
// counter (every seed of the program is a clock reading, and so are the block
// timers: the execution times print as 0) and time() as a constant
// (split_to_10's and hide_one_score's srand((int)time(0))), both inside this
// executable. std::cout is captured.
//
// The output directory holds data only. Inputs that several cases share are
// stored once: the tweet and lexicon files are those of tests/golden/uservec
// (<dir>/../uservec/{mid,tiny}_{tweets,lexicon}.csv: the same generator; the
// tool writes them where they are absent and fails where they differ from
// what it generates), the project-2 vectors are <dir>/{mid,tiny}_p2.csv. A
// case directory holds
//   cluster.conf (its relative paths point at the shared files), coins.csv;
//   expected.out: the program's output file;
//   clock.json: {"clock0", "readings", "time0"}: the first clock value, the number of
//   readings the run made, the time() constant;
//   stdout.txt (the -validate case): the line of the 10-fold value, of what the
//   program printed (the per-user progress lines before it are dropped).
// The inputs come from a counter-based generator, so a rerun reproduces every
// file byte for byte. The project-2 rows' IDs are distinct: the reference's
// k_means_pp caches distances under "<row ID>to<centroid ID>"
// (initialization.hpp:97-109), so rows sharing an ID would share distances,
// which lshkm_kmeans_pp, taking no IDs, does not reproduce.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

static long long g_clock = 0;            // the next system_clock::now() reading
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

static bool write_text(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    return fclose(f) == 0 && ok;
}

static std::string read_text(const std::string& path) {
    std::string s;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return s;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}

// -------------------------------------------------------------------- inputs
static uint64_t mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double unit(uint64_t z) { return (double)(mix(z) >> 11) * (1.0 / 9007199254740992.0); }

struct Inputs {
    std::string tweets, lexicon, coins, p2;     // the four files' text
};

// One project-2 row: the ID, then 12 values around one of 8 sign patterns
// (%.6f: general doubles after stod). The noise is wide on purpose: a clustering
// whose first k_means moves no center by min_dist_kmeans leaves dataset rows as
// the centroids, which main.cpp:109-110 then deletes.
static std::string p2_row(const std::string& id, uint64_t key, const char* eol) {
    std::string s = id;
    const int pat = (int)(mix(key) % 8);
    char buf[32];
    for (int j = 0; j < 12; j++) {
        const double base = ((pat >> (j % 3)) & 1) ? 0.5 : -0.5;
        snprintf(buf, sizeof(buf), ",%.6f", base * (1 + j / 4) + 3.0 * (unit(key * 16 + j + 1) - 0.5));
        s += buf;
    }
    return s + eol;
}

// tools/gen_uservec_golden.cpp's `tiny` (about 40 tweets, 7 users, 5 coins, CRLF
// line ends in the tweet and coin files) with coin lines of 5 fields beside
// shorter ones, and about 50 project-2 rows (CRLF) whose IDs are those tweets'
// and a few that are no tweet's.
static Inputs tiny_inputs() {
    Inputs in;
    in.coins = "bitcoin,btc,BTC,xbt,Bitcoin\r\nethereum,eth\r\nripple,xrp,XRP,rpl,Ripple,RIPPLE\r\nlitecoin,ltc\r\ndoge,dogecoin,good\r\n";
    in.lexicon = "good,1.0\ngreat,2.5\nbad,-1.5\nawful,-3.0\nmeh,0.0\nnice,0.7\r\npoor,-0.4\ngood,-9.0\nmoon,3.1\nscam,-2.2\n";
    std::string t = "P,3\r\n";
    const char* special[] = {
        "u6,s1,bad,btc", "u6,s2,awful,eth,poor", "u7,s3,meh,btc", "u7,s4,good,eth", "u1,s5,great,nice",
        "u2,s6,good,doge", "u3,s6,awful,xrp", "u1,s7,moon,BTC,bitcoin,btc", "u2,s8", "u3,s9,unknownword,ltc",
    };
    for (const char* s : special) t += std::string(s) + "\r\n";
    const char* words[] = {"good", "great", "bad", "awful", "meh", "nice", "poor", "moon", "scam", "the", "a",
                           "btc", "BTC", "eth", "xrp", "ltc", "doge", "dogecoin", "bitcoin", "ethereum"};
    for (int i = 0; i < 30; i++) {
        t += "u" + std::to_string(1 + mix(1000 + i) % 5) + ",t" + std::to_string(i);
        const int nw = 1 + (int)(mix(2000 + i) % 5);
        for (int k = 0; k < nw; k++) t += std::string(",") + words[mix(3000 + 16 * i + k) % 20];
        t += "\r\n";
    }
    in.tweets = t;
    for (int i = 0; i < 30; i++) in.p2 += p2_row("t" + std::to_string((7 * i + 3) % 30), 4100 + i, "\r\n");
    const char* rows[] = {"s1", "s3", "s4", "s5", "s6", "s7", "s8", "s9", "nosuchtweet", "t999", "s2", "x",
                          "t30", "t31", "s10", "y", "t100", "t101", "s0", "z"};
    for (int i = 0; i < 20; i++) in.p2 += p2_row(rows[i], 4200 + i, "\r\n");
    return in;
}

// tools/gen_uservec_golden.cpp's `mid` with every count times f (f = 1: about
// 3,000 tweets, 300 users, 20 coins), coin lines of 2 to 7 fields, and 1,200 f
// project-2 rows of 12 values, one in 16 of their IDs no tweet's.
static Inputs mid_inputs(int f) {
    Inputs in;
    for (int c = 0; c < 20; c++) {
        const std::string n = std::to_string(c);
        in.coins += "c" + n + ",C" + n;
        if (c % 5 == 0) in.coins += ",k" + n;
        if (c % 3 == 0) in.coins += ",a" + n + ",b" + n + ",Name" + n;      // 5 fields, 6 with the k: field 4 is Name / b
        if (c == 7) in.coins += ",q7,r7,Seven,s7,z7";                       // 7 fields
        in.coins += "\n";
    }
    char buf[64];
    for (int w = 0; w < 60; w++) {
        const double s = unit(100 + w) * 6.0 - 2.5;
        snprintf(buf, sizeof(buf), "w%d,%.6f\n", w, s);
        in.lexicon += buf;
    }
    const int T = 3000 * f, U = 300 * f;
    std::string t = "P,20\n";
    for (int i = 0; i < T; i++) {
        const int id = mix(7000 + i) % 64 == 0 && i > 10 ? (int)(mix(7500 + i) % i) : i;       // a few duplicated IDs
        t += "u" + std::to_string(mix(8000 + i) % U) + ",t" + std::to_string(id);
        const int nw = 2 + (int)(mix(9000 + i) % 4);
        for (int k = 0; k < nw; k++) {
            const uint64_t r = mix(10000 + 8 * (uint64_t)i + k);
            const int kind = (int)(r % 8);
            if (kind < 4) t += ",w" + std::to_string((r >> 8) % 60);
            else if (kind < 7) {
                const double u = (double)((r >> 8) % 1000) / 1000.0;
                t += (r >> 40) % 3 ? ",c" : ",C";
                t += std::to_string((int)(20 * u * u));                                    // skewed to the low coins
            } else t += ",x" + std::to_string((r >> 8) % 50);
        }
        t += "\n";
    }
    in.tweets = t;
    for (int i = 0; i < 1200 * f; i++) {                      // IDs 1, 3, 6, 8, ...: two of every five tweets
        const uint64_t r = mix(20000 + i);
        in.p2 += p2_row((r % 16 == 0 ? "n" : "t") + std::to_string((5 * (long long)i + 2) / 2), 30000 + (uint64_t)i, "\n");
    }
    return in;
}

struct Config {
    int p2_clusters, clusters, k, L, iters;
};

// The paths a case's configuration and command line name, relative to the case directory.
struct Paths {
    std::string p2, tweets, lexicon;
};

static std::string conf_text(const Config& c, const Paths& p) {
    std::string s;
    s += "number_of_clusters " + std::to_string(c.clusters) + "\n";
    s += "proj_2_input " + p.p2 + "\nproj_2_csv_delimiter ,\n";
    s += "proj_2_number_of_clusters " + std::to_string(c.p2_clusters) + "\n";
    s += "number_of_hash_functions " + std::to_string(c.k) + "\n";
    s += "number_of_hash_tables " + std::to_string(c.L) + "\n";
    s += "lsh_bucket_div 4\neuclidean_h_w 0.01\n";
    s += "max_algo_iterations " + std::to_string(c.iters) + "\n";
    s += "min_dist_kmeans 0.05\ncsv_delimiter 44\nlexicon_file " + p.lexicon + "\nquery_file coins.csv\n";
    return s;
}

// A file several cases share: written where absent, else it must hold `text`.
static bool shared_text(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return write_text(path, text);
    fclose(f);
    if (read_text(path) == text) return true;
    fprintf(stderr, "%s differs from what this tool generates\n", path.c_str());
    return false;
}

// Everything in `dir` (the timing run).
static bool write_inputs(const std::string& dir, const Inputs& in, const Config& c) {
    mkdir(dir.c_str(), 0777);
    const Paths p = {"p2.csv", "tweets.csv", "lex.csv"};
    return write_text(dir + "/cluster.conf", conf_text(c, p)) && write_text(dir + "/p2.csv", in.p2) &&
           write_text(dir + "/tweets.csv", in.tweets) && write_text(dir + "/lex.csv", in.lexicon) &&
           write_text(dir + "/coins.csv", in.coins);
}

// A fixture case root/name: its own configuration and coin file, the rest shared.
static bool write_case(const std::string& root, const char* name, const char* kind, const Inputs& in, const Config& c,
                       Paths* p) {
    const std::string dir = root + "/" + name, uv = root + "/../uservec", k = kind;
    mkdir(dir.c_str(), 0777);
    mkdir(uv.c_str(), 0777);
    *p = {"../" + k + "_p2.csv", "../../uservec/" + k + "_tweets.csv", "../../uservec/" + k + "_lexicon.csv"};
    return shared_text(uv + "/" + k + "_tweets.csv", in.tweets) && shared_text(uv + "/" + k + "_lexicon.csv", in.lexicon) &&
           shared_text(root + "/" + k + "_p2.csv", in.p2) && write_text(dir + "/cluster.conf", conf_text(c, *p)) &&
           write_text(dir + "/coins.csv", in.coins);
}

// The reference's main inside `dir`, the clock starting at clock0: what it
// printed, the number of clock readings, the wall seconds.
static bool run_main(const std::string& dir, const std::string& tweets, bool validate, long long clock0,
                     std::string* printed, long long* readings, double* seconds) {
    char cwd[4096];
    if (!getcwd(cwd, sizeof(cwd)) || chdir(dir.c_str()) != 0) return false;
    std::string in = tweets;
    char a0[] = "main", a1[] = "-d", a3[] = "-o", a4[] = "expected.out", a5[] = "-validate";
    char* argv[] = {a0, a1, &in[0], a3, a4, a5, nullptr};
    std::ostringstream cap;
    std::streambuf* old = std::cout.rdbuf(cap.rdbuf());
    g_clock = clock0;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    reference_main(validate ? 6 : 5, argv);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    std::cout.flush();
    std::cout.rdbuf(old);
    *readings = g_clock - clock0;
    *printed = cap.str();
    *seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    return chdir(cwd) == 0;
}

// Per block of the output file: its title and the number of user lines.
static std::string block_summary(const std::string& out) {
    std::string s;
    size_t p = 0;
    int users = -1;
    while (p < out.size()) {
        size_t e = out.find('\n', p);
        if (e == std::string::npos) e = out.size();
        const std::string line = out.substr(p, e - p);
        if (line.compare(0, 16, "Execution Time: ") == 0) { s += " " + std::to_string(users); users = -1; }
        else if (users < 0) users = 0;
        else users++;
        p = e + 1;
    }
    return s;
}

struct Case {
    const char* name;
    bool tiny, validate;
    Config conf;
};

static bool run_case(const Case& cs, const std::string& root) {
    const std::string dir = root + "/" + cs.name;
    Paths paths;
    if (!write_case(root, cs.name, cs.tiny ? "tiny" : "mid", cs.tiny ? tiny_inputs() : mid_inputs(1), cs.conf, &paths))
        return false;
    uint64_t seed = 0xC0FFEEull;
    for (const char* p = cs.name; *p; p++) seed = seed * 131 + (unsigned char)*p;
    const long long clock0 = 1000 * (long long)(seed % 1000) + 7;
    std::string printed;
    long long readings = 0;
    double seconds = 0;
    if (!run_main(dir, paths.tweets, cs.validate, clock0, &printed, &readings, &seconds)) return false;
    char js[256];
    snprintf(js, sizeof(js), "{\"clock0\": %lld, \"readings\": %lld, \"time0\": %ld}\n", clock0, readings, g_time);
    if (!write_text(dir + "/clock.json", js)) return false;
    if (cs.validate) {                              // the line of the 10-fold value (main.cpp:182)
        std::string kept;
        for (size_t p = 0; p < printed.size();) {
            size_t e = printed.find('\n', p);
            if (e == std::string::npos) e = printed.size() - 1;
            if (printed.compare(p, 3, " aa") == 0) kept += printed.substr(p, e + 1 - p);
            p = e + 1;
        }
        if (kept.empty() || !write_text(dir + "/stdout.txt", kept)) return false;
    }
    fprintf(stderr, "%s: %lld clock readings, %.2f s, user lines per block:%s\n", cs.name, readings, seconds,
            block_summary(read_text(dir + "/expected.out")).c_str());
    return true;
}

static int time_reference(int factor, const std::string& dir) {
    const Config conf = {16, 6, 4, 5, 5};
    if (!write_inputs(dir, mid_inputs(factor), conf)) return 1;
    std::string printed;
    long long readings = 0;
    double seconds = 0;
    if (!run_main(dir, "tweets.csv", false, 1, &printed, &readings, &seconds)) return 1;
    printf("{\"row\": \"main_program_reference\", \"factor\": %d, \"tweets\": %d, \"p2_rows\": %d, \"seconds\": %.3f, "
           "\"user_lines\": \"%s\"}\n", factor, 3000 * factor, 1200 * factor, seconds,
           block_summary(read_text(dir + "/expected.out")).c_str() + 1);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--time")) return time_reference(atoi(argv[2]), argv[3]);
    if (argc != 2) {
        fprintf(stderr, "usage: %s <output directory> | --time <factor> <directory>\n", argv[0]);
        return 2;
    }
    const Case cases[] = {
        {"mid", false, false, {16, 6, 4, 5, 5}},
        {"mid_skip", false, false, {12, 9, 9, 2, 5}},          // sparse tables: block B skips users
        {"mid_validate", false, true, {16, 6, 4, 5, 5}},
        {"tiny_crlf", true, false, {4, 2, 2, 2, 5}},
    };
    for (const Case& c : cases)
        if (!run_case(c, argv[1])) {
            fprintf(stderr, "cannot produce %s\n", c.name);
            return 1;
        }
    return 0;
}
