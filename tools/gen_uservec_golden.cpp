// gen_uservec_golden.cpp — golden fixtures of the user vectors from scored
// tweets, from the reference's own functions: file_to_str_vectors,
// file_to_lexicon (lib/utils.cpp:72-147), Tweet (lib/data_structures/tweet.cpp),
// the tweet map of main.cpp:128-132, tweets_to_user_vectors and
// clusters_to_user_vectors (lib/crypto_rec.hpp:78-210).
//
// Development-machine tool, not part of build(): it includes the reference's
// sources by path (REF: the reference checkout, as in oracle/Makefile; the
// binary goes outside the repository):
//
//   g++ -std=c++11 -O0 -w -I$REF -I$REF/lib -o $OUT/gen_uservec_golden tools/gen_uservec_golden.cpp \
//       $REF/lib/utils.cpp $REF/lib/data_structures/tweet.cpp $REF/lib/in_out/arg_parser.cpp
//   $OUT/gen_uservec_golden tests/golden/uservec
//   $OUT/gen_uservec_golden --time 1000000   (the baseline: seconds of clusters_to_user_vectors)
//
// Per case it writes the three input files the reference reads (<case>_tweets.csv,
// <case>_lexicon.csv, <case>_coins.csv; delimiter ','), then reads them back
// with the reference's readers and records, in <case>.npz (data only):
//   params [4] i32: P, crypto_num, user_num (the cluster count), T;
//   the tweets in the iteration order of the `tweets` map: tweet_id / user_id
//   (u1 bytes + i64 offsets [T+1] each), score [T] f64, ci_ptr [T+1] i64, ci_idx i32;
//   the clustered vectors in input order: row_id (bytes + offsets), row_cluster i32;
//   both user-vector lists (a_: tweets_to_user_vectors, b_: clusters_to_user_vectors):
//   _id (bytes + offsets), _x [n][crypto_num] f64, _mean [n] f64, _unk_ptr [n+1] i64, _unk_idx i32.
// The files are stored (uncompressed) zips with zeroed timestamps and the
// inputs come from a counter-based generator, so a rerun reproduces every file
// byte for byte.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

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
    // a list of strings: <n> u1 bytes concatenated, <n>_off i64 offsets
    void strs(const std::string& n, const std::vector<std::string>& v) {
        std::string b;
        std::vector<int64_t> off(1, 0);
        for (const std::string& s : v) { b += s; off.push_back((int64_t)b.size()); }
        add(n, "|u1", {b.size()}, b.data(), b.size());
        i64(n + "_off", off);
    }
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

static bool write_text(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    fclose(f);
    return ok;
}

// -------------------------------------------------------------------- inputs
static uint64_t mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Inputs {
    std::string tweets, lexicon, coins;                 // the three files' text
    std::vector<std::string> row_id;                    // the clustered vectors, in input order
    std::vector<int32_t> row_cluster;
    int user_num;
};

// About 40 tweets, 7 users, 5 coins, about 50 clustered IDs over 4 clusters, with
// every special case written out. CRLF line ends in the tweet and coin files
// (the lexicon reader does not strip '\r': stof stops at it).
static Inputs tiny_inputs() {
    Inputs in;
    in.coins = "bitcoin,btc,BTC\r\nethereum,eth\r\nripple,xrp\r\nlitecoin,ltc\r\ndoge,dogecoin,good\r\n";   // "good": the lexicon wins
    in.lexicon = "good,1.0\ngreat,2.5\nbad,-1.5\nawful,-3.0\nmeh,0.0\nnice,0.7\r\npoor,-0.4\ngood,-9.0\nmoon,3.1\nscam,-2.2\n";
    std::string t = "P,3\r\n";
    const char* special[] = {
        "u6,s1,bad,btc",                 // u6: only scores <= 0 -> dropped
        "u6,s2,awful,eth,poor",
        "u7,s3,meh,btc",                 // u7: a zero-score known coin ...
        "u7,s4,good,eth",                // ... and a positive one
        "u1,s5,great,nice",              // no coin
        "u2,s6,good,doge",               // "good" is a lexicon word here, "doge" the coin
        "u3,s6,awful,xrp",               // duplicated tweet ID: the first wins
        "u1,s7,moon,BTC,bitcoin,btc",    // three variations of one coin
        "u2,s8",                         // no word at all
        "u3,s9,unknownword,ltc",         // score 0 / sqrt(15) = 0
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
    in.user_num = 4;                                     // cluster 2 stays empty
    const int cl[3] = {0, 1, 3};
    for (int i = 0; i < 30; i++) {
        in.row_id.push_back("t" + std::to_string((int)(mix(4000 + i) % 30)));    // repeats: one tweet on several rows
        in.row_cluster.push_back(cl[mix(5000 + i) % 3]);
    }
    const char* rows[] = {"s1", "s3", "s4", "s5", "s6", "s7", "s7", "s8", "s9", "nosuchtweet", "t999", "s2",
                          "t3", "t3", "s4", "x", "t11", "t12", "s6", "t29"};
    for (int i = 0; i < 20; i++) {
        in.row_id.push_back(rows[i]);
        in.row_cluster.push_back(cl[mix(6000 + i) % 3]);
    }
    return in;
}

// About 3,000 tweets, 300 users, 20 coins, 16 clusters: both maps rehash several times.
static Inputs mid_inputs() {
    Inputs in;
    for (int c = 0; c < 20; c++) {
        in.coins += "c" + std::to_string(c) + ",C" + std::to_string(c);
        if (c % 5 == 0) in.coins += ",k" + std::to_string(c);
        in.coins += "\n";
    }
    char buf[64];
    for (int w = 0; w < 60; w++) {
        // scores in (-2.5, 3.5): mostly positive totals, full float mantissas after stof
        const double s = (double)(mix(100 + w) >> 11) * (1.0 / 9007199254740992.0) * 6.0 - 2.5;
        snprintf(buf, sizeof(buf), "w%d,%.6f\n", w, s);
        in.lexicon += buf;
    }
    std::string t = "P,20\n";
    for (int i = 0; i < 3000; i++) {
        const int id = mix(7000 + i) % 64 == 0 && i > 10 ? (int)(mix(7500 + i) % i) : i;       // a few duplicated IDs
        t += "u" + std::to_string(mix(8000 + i) % 300) + ",t" + std::to_string(id);
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
    in.user_num = 16;
    for (int i = 0; i < 3200; i++) {
        const uint64_t r = mix(20000 + i);
        in.row_id.push_back((r % 16 == 0 ? "n" : "t") + std::to_string((r >> 8) % 3000));
        in.row_cluster.push_back((int32_t)((r >> 32) % 16));
    }
    return in;
}

static void record_users(Npz& z, const std::string& p, std::vector<Vec>& us, int C) {
    std::vector<std::string> ids;
    std::vector<double> x, mean;
    std::vector<int64_t> up(1, 0);
    std::vector<int32_t> ui;
    for (Vec& u : us) {
        ids.push_back(u.getId());
        for (int j = 0; j < C; j++) x.push_back(u.getDimensions()->at(j));
        mean.push_back(u.getKnownMean());
        for (int j : u.getUnknownIndexesSet()) ui.push_back(j);
        up.push_back((int64_t)ui.size());
    }
    z.strs(p + "id", ids);
    z.f64(p + "x", x, {us.size(), (size_t)C});
    z.f64(p + "mean", mean);
    z.i64(p + "unk_ptr", up);
    z.i32(p + "unk_idx", ui);
}

static bool run_case(const char* name, const Inputs& in, const std::string& dir) {
    const std::string base = dir + "/" + name;
    if (!write_text(base + "_tweets.csv", in.tweets) || !write_text(base + "_lexicon.csv", in.lexicon) ||
        !write_text(base + "_coins.csv", in.coins))
        return false;
    // main.cpp:120-137
    int P = 1;
    vector< vector<string> > input_tweets = file_to_str_vectors(base + "_tweets.csv", ',', &P);
    vector< vector<string> > query_crypto = file_to_str_vectors(base + "_coins.csv", ',');
    unordered_map<string, float> lexicon = file_to_lexicon(base + "_lexicon.csv", ',');
    unordered_map<string, Tweet> tweets;
    for (auto& tweet_words : input_tweets) {
        Tweet tweetWStats(tweet_words, lexicon, query_crypto);
        tweets.emplace(tweetWStats.getId(), tweetWStats);
    }
    std::vector<Vec> clustered;
    for (size_t i = 0; i < in.row_id.size(); i++) {
        Vec v(in.row_id[i], std::vector<double>());
        v.setCluster(in.row_cluster[i], 0.0);
        clustered.push_back(v);
    }
    const int C = (int)query_crypto.size();
    std::vector<Vec> user_vectors = tweets_to_user_vectors<double>(tweets, C);
    std::vector<Vec> fake_user_vectors = clusters_to_user_vectors(tweets, clustered, C, in.user_num);

    Npz z;
    z.i32("params", {P, C, in.user_num, (int32_t)tweets.size()});
    std::vector<std::string> tid, uid;
    std::vector<double> score;
    std::vector<int64_t> cp(1, 0);
    std::vector<int32_t> ci;
    for (auto& kv : tweets) {
        tid.push_back(kv.second.getId());
        uid.push_back(kv.second.getUserId());
        score.push_back(kv.second.getSentimentScore());
        for (int j : kv.second.getCryptoIndexes()) ci.push_back(j);
        cp.push_back((int64_t)ci.size());
    }
    z.strs("tweet_id", tid);
    z.strs("user_id", uid);
    z.f64("score", score);
    z.i64("ci_ptr", cp);
    z.i32("ci_idx", ci);
    z.strs("row_id", in.row_id);
    z.i32("row_cluster", in.row_cluster);
    record_users(z, "a_", user_vectors, C);
    record_users(z, "b_", fake_user_vectors, C);
    fprintf(stderr, "%s: P %d, %zu lines, %zu tweets, %d coins, %zu mentions, %zu users kept, %zu of %d clusters kept\n", name,
            P, input_tweets.size(), tweets.size(), C, ci.size(), user_vectors.size(), fake_user_vectors.size(), in.user_num);
    return z.write(base + ".npz");
}

// The baseline: clusters_to_user_vectors itself on N tweets shaped like the C5
// shard (K = 1024 clusters, 100 coins, 1 or 2 coins per tweet drawn as
// floor(100 u^3), about four fifths of the scores positive), every clustered
// vector a tweet, on this one core. tools/uservec_time.py draws the same shape.
static int time_reference(int N) {
    const int C = 100, K = 1024;
    vector< vector<string> > query_crypto;
    for (int c = 0; c < C; c++) query_crypto.push_back({"c" + std::to_string(c)});
    unordered_map<string, float> lexicon;
    for (int w = 0; w < 64; w++) lexicon.emplace("w" + std::to_string(w), (float)((double)(mix(w) >> 40) / 16777216.0 * 5.0 - 1.0));
    unordered_map<string, Tweet> tweets;
    std::vector<Vec> clustered;
    clustered.reserve(N);
    for (int i = 0; i < N; i++) {
        const uint64_t r = mix(0xC5000000ull + i);
        vector<string> words = {"u" + std::to_string(r % 100000), "t" + std::to_string(i), "w" + std::to_string((r >> 20) % 64)};
        const int nc = 1 + (int)((r >> 30) & 1);
        for (int k = 0; k < nc; k++) {
            const double u = (double)(mix(r + k) >> 11) * (1.0 / 9007199254740992.0);
            words.push_back("c" + std::to_string((int)(C * u * u * u)));
        }
        Tweet tw(words, lexicon, query_crypto);
        tweets.emplace(tw.getId(), tw);
        Vec v(words[1], std::vector<double>());
        v.setCluster((int)((r >> 40) % K), 0.0);
        clustered.push_back(v);
    }
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    std::vector<Vec> fake = clusters_to_user_vectors(tweets, clustered, C, K);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    printf("{\"row\": \"uservec_reference\", \"visits\": %d, \"K\": %d, \"coins\": %d, \"seconds\": %.3f, \"kept\": %zu}\n", N, K, C,
           (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec), fake.size());
    return 0;
}

int main(int argc, char** argv) {
    std::cout.setstate(std::ios_base::failbit);      // the reference's progress lines
    if (argc == 3 && !strcmp(argv[1], "--time")) return time_reference(atoi(argv[2]));
    if (argc != 2) {
        fprintf(stderr, "usage: %s <output directory> | --time <N>\n", argv[0]);
        return 2;
    }
    if (!run_case("tiny", tiny_inputs(), argv[1]) || !run_case("mid", mid_inputs(), argv[1])) {
        fprintf(stderr, "cannot write the fixtures\n");
        return 1;
    }
    return 0;
}
