// tweets.cpp — the reference's tweet, lexicon and coin formats and the order
// in which it visits tweets and users, host side.
//
//   file_to_str_vectors        lib/utils.cpp:72-127
//   file_to_lexicon            lib/utils.cpp:130-147
//   Tweet::Tweet               lib/data_structures/tweet.cpp:11-42
//   the tweet map              main.cpp:128-132
//   tweets_to_user_vectors     lib/crypto_rec.hpp:84-103 (the user map's order)
//   print_recommendations      main.cpp:557-569 and the blocks' lines, :151-173
//
// Everything after main.cpp:132 iterates std::unordered_map<std::string, ...>,
// so the order of the tweets and of the users is libstdc++'s hash order. It is
// obtained here by doing what the reference does: real unordered_maps keyed by
// the same strings, filled by the same insertion sequence (the order depends on
// the keys, the insertion order and the rehash policy, not on the mapped type).
// Lines are scored in parallel; the maps are filled sequentially.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/lshkm.h"
#include "common.h"

using namespace lshkm;

namespace {

int slurp(const char* path, std::string* data) {
    std::ifstream f(path, std::ios::binary);
    if (!f.is_open()) return -1;
    f.seekg(0, std::ios::end);
    const std::streamoff n = f.tellg();
    f.seekg(0, std::ios::beg);
    data->resize((size_t)std::max<std::streamoff>(n, 0));
    if (n > 0) f.read(&(*data)[0], n);
    return 0;
}

// getline(file, line): no line after a final '\n'
std::vector<std::string> lines_of(const std::string& data) {
    std::vector<std::string> out;
    size_t p = 0;
    while (p < data.size()) {
        size_t e = data.find('\n', p);
        if (e == std::string::npos) e = data.size();
        out.push_back(data.substr(p, e - p));
        p = e + 1;
    }
    return out;
}

// split (utils.cpp:11-19): getline semantics, no token after a trailing delimiter
std::vector<std::string> split(const std::string& s, char delim) {
    std::vector<std::string> tok;
    size_t i = 0;
    while (i < s.size()) {
        size_t j = s.find(delim, i);
        if (j == std::string::npos) j = s.size();
        tok.push_back(s.substr(i, j - i));
        i = j + 1;
    }
    return tok;
}

// file_to_str_vectors' line: one trailing '\r' dropped, then split
std::vector<std::string> str_vector(std::string line, char delim) {
    if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
    return split(line, delim);
}

// std::stof (libstdc++ __stoa over strtof): invalid_argument when nothing
// parses, out_of_range whenever strtof sets ERANGE.
int stof_like(const std::string& s, float* out) {
    const char* b = s.c_str();
    char* e = nullptr;
    errno = 0;
    const float v = strtof(b, &e);
    if (e == b || errno == ERANGE) return -1;
    *out = v;
    return 0;
}

int stoi_like(const std::string& s, int* out) {
    const char* b = s.c_str();
    char* e = nullptr;
    errno = 0;
    const long v = strtol(b, &e, 10);
    if (e == b || errno == ERANGE || v > 2147483647L || v < -2147483647L - 1) return -1;
    *out = (int)v;
    return 0;
}

std::string at_line(const char* path, size_t line) { return std::string(path) + ":" + std::to_string(line) + ": "; }

struct Scored {
    double score;
    std::vector<int32_t> coins;      // the std::set<int>'s order
};

}  // namespace

struct lshkm_tweets_s {
    int P = 1;
    int crypto_num = 0;
    // tweets in the iteration order of the reference's `tweets` map
    std::vector<std::string> tid;
    std::vector<double> score;
    std::vector<int64_t> ci_ptr;
    std::vector<int32_t> ci_idx;
    std::vector<int32_t> user_of;
    // users in the iteration order of the reference's `user_map`
    std::vector<std::string> uid;
    std::unordered_map<std::string, int32_t> number;      // tweet ID -> its number
    std::vector<std::vector<std::string>> coin_fields;    // query_crypto: the coin file's lines, split
};

extern "C" {

int lshkm_tweets_read(const char* input_path, const char* lexicon_path, const char* query_path, char delimiter,
                      int threads, lshkm_tweets* out) {
    LSHKM_CHECK(input_path && lexicon_path && query_path && out, LSHKM_ERR_ARG, "bad arguments");
    std::string in_data, lex_data, q_data;
    // the reference goes on with an empty table where a file does not open
    LSHKM_CHECK(slurp(input_path, &in_data) == 0, LSHKM_ERR_ARG, std::string("cannot open ") + input_path);
    LSHKM_CHECK(slurp(lexicon_path, &lex_data) == 0, LSHKM_ERR_ARG, std::string("cannot open ") + lexicon_path);
    LSHKM_CHECK(slurp(query_path, &q_data) == 0, LSHKM_ERR_ARG, std::string("cannot open ") + query_path);

    // file_to_lexicon: no '\r' handling (stof stops at it); the first occurrence of a word wins
    std::unordered_map<std::string, float> lexicon;
    {
        const std::vector<std::string> ls = lines_of(lex_data);
        for (size_t i = 0; i < ls.size(); i++) {
            const std::vector<std::string> w = split(ls[i], delimiter);
            LSHKM_CHECK(w.size() >= 2, LSHKM_ERR_ARG,
                        at_line(lexicon_path, i + 1) + "fewer than two tokens (the reference reads current_word[1])");
            float s;
            LSHKM_CHECK(stof_like(w[1], &s) == 0, LSHKM_ERR_ARG,
                        at_line(lexicon_path, i + 1) + "std::stof(\"" + w[1] + "\") would throw");
            lexicon.emplace(w[0], s);
        }
    }
    // the coin file: one coin per line, every token a variation. The reference
    // compares a word with every variation of every coin (tweet.cpp:28-35); the
    // same matches, by variation.
    std::unordered_map<std::string, std::vector<int32_t>> coin_of;
    int crypto_num = 0;
    std::vector<std::vector<std::string>> coin_fields;
    {
        const std::vector<std::string> ls = lines_of(q_data);
        coin_fields.reserve(ls.size());
        for (const std::string& l : ls) {
            coin_fields.push_back(str_vector(l, delimiter));
            for (const std::string& var : coin_fields.back()) {
                std::vector<int32_t>& v = coin_of[var];
                if (v.empty() || v.back() != crypto_num) v.push_back(crypto_num);
            }
            crypto_num++;
        }
    }
    // the tweet file: P from the first line's second token, then one tweet per line
    std::vector<std::string> ls = lines_of(in_data);
    int P = 1;
    if (!ls.empty()) {
        const std::vector<std::string> head = str_vector(ls[0], delimiter);
        if (head.size() > 1)
            LSHKM_CHECK(stoi_like(head[1], &P) == 0, LSHKM_ERR_ARG,
                        at_line(input_path, 1) + "std::stoi(\"" + head[1] + "\") would throw");
    }
    const size_t n_lines = ls.size() > 1 ? ls.size() - 1 : 0;
    std::vector<std::vector<std::string>> words(n_lines);
    std::vector<Scored> sc(n_lines);
    // threads <= 0: the hardware's, one per 256 lines at most
    int nt = threads > 0 ? threads
                         : (int)std::min<size_t>(std::max(1u, std::thread::hardware_concurrency()), n_lines / 256 + 1);
    nt = (int)std::min<size_t>((size_t)std::min(nt, 64), std::max<size_t>(n_lines, 1));
    std::vector<size_t> bad(nt, 0);                       // 1-based file line of the first short line, per slice
    auto work = [&](int t) {
        const size_t lo = n_lines * t / nt, hi = n_lines * (t + 1) / nt;
        for (size_t i = lo; i < hi; i++) {
            words[i] = str_vector(ls[i + 1], delimiter);
            const std::vector<std::string>& w = words[i];
            if (w.size() < 2) { if (!bad[t]) bad[t] = i + 2; continue; }
            // Tweet::Tweet: double + float in word order; a lexicon word is never a coin
            double totalscore = 0;
            std::set<int> coins;
            for (size_t k = 2; k < w.size(); k++) {
                auto lx = lexicon.find(w[k]);
                if (lx != lexicon.end()) {
                    totalscore = totalscore + lx->second;
                } else {
                    auto c = coin_of.find(w[k]);
                    if (c != coin_of.end()) coins.insert(c->second.begin(), c->second.end());
                }
            }
            const int alpha = 15;
            sc[i].score = totalscore / sqrt(totalscore * totalscore + alpha);
            sc[i].coins.assign(coins.begin(), coins.end());
        }
    };
    {
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
    }
    for (int t = 0; t < nt; t++)
        LSHKM_CHECK(!bad[t], LSHKM_ERR_ARG,
                    at_line(input_path, bad[t]) + "fewer than two tokens (the reference reads tweet_words[1])");

    // main.cpp:128-132: emplace in file order, the first tweet of an ID wins
    std::unordered_map<std::string, int32_t> tweets;
    for (size_t i = 0; i < n_lines; i++) tweets.emplace(words[i][1], (int32_t)i);
    lshkm_tweets t = new lshkm_tweets_s();
    t->P = P;
    t->crypto_num = crypto_num;
    t->coin_fields.swap(coin_fields);
    const size_t T = tweets.size();
    t->tid.reserve(T);
    t->score.reserve(T);
    t->user_of.reserve(T);
    t->ci_ptr.reserve(T + 1);
    t->ci_ptr.push_back(0);
    // crypto_rec.hpp:84-95: users are emplaced while walking the tweet map
    std::unordered_map<std::string, int32_t> user_map;
    std::vector<const std::string*> tweet_user;
    tweet_user.reserve(T);
    for (auto& kv : tweets) {
        const size_t line = (size_t)kv.second;
        t->tid.push_back(kv.first);
        t->score.push_back(sc[line].score);
        t->ci_idx.insert(t->ci_idx.end(), sc[line].coins.begin(), sc[line].coins.end());
        t->ci_ptr.push_back((int64_t)t->ci_idx.size());
        auto u = user_map.emplace(words[line][0], 0).first;
        tweet_user.push_back(&u->first);                 // node keys do not move on rehash
    }
    // crypto_rec.hpp:107: the user map's own iteration order numbers the slots
    t->uid.reserve(user_map.size());
    for (auto& kv : user_map) {
        kv.second = (int32_t)t->uid.size();
        t->uid.push_back(kv.first);
    }
    for (size_t i = 0; i < T; i++) t->user_of.push_back(user_map.find(*tweet_user[i])->second);
    t->number.reserve(T);
    for (size_t i = 0; i < T; i++) t->number.emplace(t->tid[i], (int32_t)i);
    *out = t;
    return 0;
}

int lshkm_tweets_info(lshkm_tweets t, int* P, int64_t* n_tweets, int64_t* n_users, int* crypto_num, int64_t* mentions,
                      int64_t* id_bytes, int64_t* user_id_bytes) {
    LSHKM_CHECK(t, LSHKM_ERR_ARG, "tweets is NULL");
    int64_t ib = 0, ub = 0;
    for (const std::string& s : t->tid) ib += (int64_t)s.size();
    for (const std::string& s : t->uid) ub += (int64_t)s.size();
    if (P) *P = t->P;
    if (n_tweets) *n_tweets = (int64_t)t->tid.size();
    if (n_users) *n_users = (int64_t)t->uid.size();
    if (crypto_num) *crypto_num = t->crypto_num;
    if (mentions) *mentions = (int64_t)t->ci_idx.size();
    if (id_bytes) *id_bytes = ib;
    if (user_id_bytes) *user_id_bytes = ub;
    return 0;
}

int lshkm_tweets_table(lshkm_tweets t, double* score_host, int64_t* ci_ptr_host, int32_t* ci_idx_host,
                       int32_t* user_of_host) {
    LSHKM_CHECK(t, LSHKM_ERR_ARG, "tweets is NULL");
    if (score_host && !t->score.empty()) std::memcpy(score_host, t->score.data(), 8 * t->score.size());
    if (ci_ptr_host) std::memcpy(ci_ptr_host, t->ci_ptr.data(), 8 * t->ci_ptr.size());
    if (ci_idx_host && !t->ci_idx.empty()) std::memcpy(ci_idx_host, t->ci_idx.data(), 4 * t->ci_idx.size());
    if (user_of_host && !t->user_of.empty()) std::memcpy(user_of_host, t->user_of.data(), 4 * t->user_of.size());
    return 0;
}

static int ids_out(const std::vector<std::string>& ids, char* bytes_host, int64_t* offsets_host) {
    LSHKM_CHECK(offsets_host && (bytes_host || ids.empty()), LSHKM_ERR_ARG, "bad arguments");
    int64_t o = 0;
    offsets_host[0] = 0;
    for (size_t i = 0; i < ids.size(); i++) {
        std::memcpy(bytes_host + o, ids[i].data(), ids[i].size());
        o += (int64_t)ids[i].size();
        offsets_host[i + 1] = o;
    }
    return 0;
}

int lshkm_tweets_ids(lshkm_tweets t, char* bytes_host, int64_t* offsets_host) {
    LSHKM_CHECK(t, LSHKM_ERR_ARG, "tweets is NULL");
    return ids_out(t->tid, bytes_host, offsets_host);
}

int lshkm_tweets_user_ids(lshkm_tweets t, char* bytes_host, int64_t* offsets_host) {
    LSHKM_CHECK(t, LSHKM_ERR_ARG, "tweets is NULL");
    return ids_out(t->uid, bytes_host, offsets_host);
}

int lshkm_tweets_match(lshkm_tweets t, const char* id_bytes, const int64_t* id_offsets, int64_t n,
                       int32_t* tweet_of_row_host) {
    LSHKM_CHECK(t && n >= 0 && (n == 0 || (id_offsets && tweet_of_row_host)), LSHKM_ERR_ARG, "bad arguments");
    for (int64_t i = 0; i < n; i++) {
        LSHKM_CHECK(id_offsets[i + 1] >= id_offsets[i] && (id_bytes || id_offsets[i + 1] == id_offsets[i]), LSHKM_ERR_ARG,
                    "bad ID offsets");
        const std::string id(id_bytes ? id_bytes + id_offsets[i] : "", (size_t)(id_offsets[i + 1] - id_offsets[i]));
        auto it = t->number.find(id);
        tweet_of_row_host[i] = it == t->number.end() ? -1 : it->second;
    }
    return 0;
}

// print_recommendations' choice (main.cpp:563-566); a line without a field has no name
static const std::string& coin_name(const lshkm_tweets_s* t, int32_t coin, int name_index) {
    static const std::string none;
    const std::vector<std::string>& f = t->coin_fields[(size_t)coin];
    if (f.size() > (size_t)name_index) return f[(size_t)name_index];
    return f.empty() ? none : f[0];
}

int lshkm_tweets_coin_names(lshkm_tweets t, int name_index, char* bytes_host, int64_t* offsets_host) {
    LSHKM_CHECK(t && name_index >= 0 && offsets_host, LSHKM_ERR_ARG, "bad arguments");
    int64_t o = 0;
    offsets_host[0] = 0;
    for (int32_t c = 0; c < t->crypto_num; c++) {
        const std::string& s = coin_name(t, c, name_index);
        if (bytes_host) std::memcpy(bytes_host + o, s.data(), s.size());
        o += (int64_t)s.size();
        offsets_host[c + 1] = o;
    }
    return 0;
}

int lshkm_recom_write(lshkm_tweets t, int name_index, const char* path, int append, const char* title,
                      const char* user_id_bytes, const int64_t* user_id_offsets, int64_t nq, const int32_t* top_host,
                      int n_top, const uint8_t* skip_host, int64_t elapsed_ms) {
    LSHKM_CHECK(t && name_index >= 0 && path && title && nq >= 0 && n_top >= 0, LSHKM_ERR_ARG, "bad arguments");
    LSHKM_CHECK(nq == 0 || (user_id_offsets && (top_host || n_top == 0)), LSHKM_ERR_ARG, "bad arguments");
    // everything is checked before the file is touched
    for (int64_t q = 0; q < nq; q++) {
        LSHKM_CHECK(user_id_offsets[q + 1] >= user_id_offsets[q] && (user_id_bytes || user_id_offsets[q + 1] == user_id_offsets[q]),
                    LSHKM_ERR_ARG, "bad ID offsets");
        if (skip_host && skip_host[q]) continue;
        for (int j = 0; j < n_top; j++) {
            const int32_t c = top_host[q * n_top + j];
            LSHKM_CHECK(c >= 0 && c < t->crypto_num, LSHKM_ERR_ARG,
                        "user " + std::to_string(q) + ": coin index " + std::to_string(c) + " outside [0, " +
                            std::to_string(t->crypto_num) + ")");
        }
    }
    std::string out = std::string(title) + "\n";
    for (int64_t q = 0; q < nq; q++) {
        if (skip_host && skip_host[q]) continue;
        if (user_id_offsets[q + 1] > user_id_offsets[q])
            out.append(user_id_bytes + user_id_offsets[q], (size_t)(user_id_offsets[q + 1] - user_id_offsets[q]));
        for (int j = 0; j < n_top; j++) {
            out.push_back(' ');
            out += coin_name(t, top_host[q * n_top + j], name_index);
        }
        out.push_back('\n');
    }
    out += "Execution Time: " + std::to_string((long long)elapsed_ms) + "\n";
    FILE* f = fopen(path, append ? "ab" : "wb");
    LSHKM_CHECK(f, LSHKM_ERR_ARG, std::string("cannot open ") + path + " for writing");
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    const bool closed = fclose(f) == 0;
    LSHKM_CHECK(ok && closed, LSHKM_ERR_ARG, std::string("cannot write ") + path);
    return 0;
}

int lshkm_tweets_free(lshkm_tweets t) {
    delete t;
    return 0;
}

}  // extern "C"
