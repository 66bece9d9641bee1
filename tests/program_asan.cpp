// program_asan.cpp — the printers of liblshkm (lshkm_tweets_coin_names and
// lshkm_recom_write, csrc/tweets.cpp) built with -fsanitize=address,undefined
// as a stand-alone host program and run over the committed `tiny_crlf` case:
// the names at several name indexes, the reference's output file parsed and
// written back byte for byte, skipped users, the refusals (an index out of
// range, a path that cannot be opened) and the empty shapes. Driven by
// tests/test_program_cpu.py; any sanitizer report fails the run.
//
//   program_asan <tmpdir> <tweets.csv> <lex.csv> <coins.csv> <expected.out>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../crypto-recommendation_amd/csrc/tweets.cpp"

namespace lshkm {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace lshkm

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #c, lshkm::g_err.c_str()); failures++; } } while (0)

static std::string read_file(const std::string& p) {
    std::string s;
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return s;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}

static std::vector<std::string> names_at(lshkm_tweets t, int C, int name_index) {
    std::vector<int64_t> off((size_t)C + 1);
    EXPECT(lshkm_tweets_coin_names(t, name_index, nullptr, off.data()) == 0);       // the sizes alone
    std::vector<char> bytes((size_t)off[(size_t)C]);                                 // exactly as many bytes
    std::vector<int64_t> off2((size_t)C + 1);
    EXPECT(lshkm_tweets_coin_names(t, name_index, bytes.data(), off2.data()) == 0);
    EXPECT(off == off2);
    std::vector<std::string> out;
    for (int c = 0; c < C; c++) out.emplace_back(bytes.data() + off[(size_t)c], (size_t)(off[(size_t)c + 1] - off[(size_t)c]));
    return out;
}

struct Block {
    std::string title, ids;
    std::vector<int64_t> off{0};
    std::vector<int32_t> top;
    int n_top = 0;
};

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const std::string tmp = argv[1], want = read_file(argv[5]);
    lshkm_tweets t = nullptr;
    EXPECT(lshkm_tweets_read(argv[2], argv[3], argv[4], ',', 2, &t) == 0);
    if (!t) return 1;
    int C = 0;
    lshkm_tweets_info(t, nullptr, nullptr, nullptr, &C, nullptr, nullptr, nullptr);
    EXPECT(C == 5);

    // the names: field 4 of the long lines, field 0 of the others
    const std::vector<std::string> names = names_at(t, C, 4);
    EXPECT(names[0] == "Bitcoin" && names[1] == "ethereum" && names[2] == "Ripple" && names[3] == "litecoin" && names[4] == "doge");
    EXPECT(names_at(t, C, 0)[2] == "ripple" && names_at(t, C, 5)[2] == "RIPPLE" && names_at(t, C, 5)[0] == "bitcoin");
    EXPECT(names_at(t, C, 2147483647)[4] == "doge");
    int64_t one = 0;
    EXPECT(lshkm_tweets_coin_names(t, -1, nullptr, &one) == LSHKM_ERR_ARG);
    EXPECT(lshkm_tweets_coin_names(t, 4, nullptr, nullptr) == LSHKM_ERR_ARG);
    EXPECT(lshkm_tweets_coin_names(nullptr, 4, nullptr, &one) == LSHKM_ERR_ARG);

    // the reference's file, parsed and written back
    std::map<std::string, int32_t> index;
    for (int c = 0; c < C; c++) index[names[(size_t)c]] = c;
    std::vector<Block> blocks;
    {
        bool open = false;
        for (const std::string& ln : lines_of(want)) {
            if (!open) { blocks.emplace_back(); blocks.back().title = ln; open = true; continue; }
            if (ln.compare(0, 16, "Execution Time: ") == 0) { open = false; continue; }
            const std::vector<std::string> f = split(ln, ' ');
            Block& b = blocks.back();
            b.ids += f[0];
            b.off.push_back((int64_t)b.ids.size());
            b.n_top = (int)f.size() - 1;
            for (size_t j = 1; j < f.size(); j++) b.top.push_back(index.at(f[j]));
        }
    }
    EXPECT(blocks.size() == 4);
    const std::string out = tmp + "/out.txt";
    for (size_t b = 0; b < blocks.size(); b++) {
        const Block& k = blocks[b];
        EXPECT(lshkm_recom_write(t, 4, out.c_str(), b > 0, k.title.c_str(), k.ids.data(), k.off.data(),
                                 (int64_t)k.off.size() - 1, k.top.data(), k.n_top, nullptr, 0) == 0);
    }
    EXPECT(read_file(out) == want);

    // skipped users: their rows are not read (out-of-range values) and not printed
    const char ids[] = "abbccc";
    const int64_t off[] = {0, 1, 3, 6};
    int32_t top[] = {0, 4, -1, 99, 2, 2};
    const uint8_t skip[] = {0, 1, 0};
    EXPECT(lshkm_recom_write(t, 4, out.c_str(), 0, "T", ids, off, 3, top, 2, skip, 7) == 0);
    EXPECT(read_file(out) == "T\na Bitcoin doge\nccc Ripple Ripple\nExecution Time: 7\n");
    // refusals leave the file as it is
    const uint8_t none[] = {0, 0, 0};
    EXPECT(lshkm_recom_write(t, 4, out.c_str(), 0, "T", ids, off, 3, top, 2, none, 7) == LSHKM_ERR_ARG);
    EXPECT(lshkm::g_err.find("outside [0, 5)") != std::string::npos);
    top[2] = 0;
    top[3] = C;
    EXPECT(lshkm_recom_write(t, 4, out.c_str(), 1, "T", ids, off, 3, top, 2, nullptr, 7) == LSHKM_ERR_ARG);
    const int64_t bad_off[] = {0, 3, 1, 6};
    EXPECT(lshkm_recom_write(t, 4, out.c_str(), 1, "T", ids, bad_off, 3, top, 2, skip, 7) == LSHKM_ERR_ARG);
    EXPECT(lshkm_recom_write(t, 4, (tmp + "/absent/out.txt").c_str(), 0, "T", ids, off, 3, top, 2, skip, 7) == LSHKM_ERR_ARG);
    EXPECT(lshkm::g_err.find("absent") != std::string::npos);
    EXPECT(lshkm_recom_write(t, 4, tmp.c_str(), 1, "T", ids, off, 3, top, 2, skip, 7) == LSHKM_ERR_ARG);      // a directory
    EXPECT(lshkm_recom_write(t, 4, nullptr, 1, "T", ids, off, 3, top, 2, skip, 7) == LSHKM_ERR_ARG);
    EXPECT(lshkm_recom_write(t, 4, out.c_str(), 1, nullptr, ids, off, 3, top, 2, skip, 7) == LSHKM_ERR_ARG);
    EXPECT(lshkm_recom_write(t, 4, out.c_str(), 1, "T", ids, off, 3, nullptr, 2, skip, 7) == LSHKM_ERR_ARG);
    EXPECT(read_file(out) == "T\na Bitcoin doge\nccc Ripple Ripple\nExecution Time: 7\n");
    // the empty shapes: no user; users without a coin; empty IDs
    EXPECT(lshkm_recom_write(t, 4, out.c_str(), 0, "", nullptr, nullptr, 0, nullptr, 5, nullptr, 0) == 0);
    EXPECT(read_file(out) == "\nExecution Time: 0\n");
    const int64_t off0[] = {0, 0, 1};
    EXPECT(lshkm_recom_write(t, 4, out.c_str(), 1, "T", ids, off0, 2, nullptr, 0, nullptr, -3) == 0);
    EXPECT(read_file(out) == "\nExecution Time: 0\nT\n\na\nExecution Time: -3\n");
    lshkm_tweets_free(t);

    // a coin file with an empty line: the reference reads out of bounds there; the name is empty
    {
        FILE* f = fopen((tmp + "/coins").c_str(), "wb");
        fputs("bitcoin,btc\n\nethereum,eth,a,b,Ether\n", f);
        fclose(f);
        FILE* g = fopen((tmp + "/empty").c_str(), "wb");
        fclose(g);
        lshkm_tweets u = nullptr;
        EXPECT(lshkm_tweets_read((tmp + "/empty").c_str(), (tmp + "/empty").c_str(), (tmp + "/coins").c_str(), ',', 1, &u) == 0);
        if (u) {
            const std::vector<std::string> n = names_at(u, 3, 4);
            EXPECT(n[0] == "bitcoin" && n[1] == "" && n[2] == "Ether");
            const int32_t tp[] = {1, 2};
            const int64_t o1[] = {0, 1};
            EXPECT(lshkm_recom_write(u, 4, out.c_str(), 0, "T", "u", o1, 1, tp, 2, nullptr, 1) == 0);
            EXPECT(read_file(out) == "T\nu  Ether\nExecution Time: 1\n");
            lshkm_tweets_free(u);
        }
        lshkm_tweets e = nullptr;
        EXPECT(lshkm_tweets_read((tmp + "/empty").c_str(), (tmp + "/empty").c_str(), (tmp + "/empty").c_str(), ',', 1, &e) == 0);
        if (e) {
            int64_t o = -1;
            EXPECT(lshkm_tweets_coin_names(e, 4, nullptr, &o) == 0 && o == 0);
            const int32_t tp[] = {0};
            const int64_t o1[] = {0, 1};
            EXPECT(lshkm_recom_write(e, 4, out.c_str(), 0, "T", "u", o1, 1, tp, 1, nullptr, 1) == LSHKM_ERR_ARG);    // no coin at all
            lshkm_tweets_free(e);
        }
    }

    if (failures) return 1;
    printf("program_asan ok\n");
    return 0;
}
