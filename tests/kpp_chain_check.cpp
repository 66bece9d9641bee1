// Host check of crypto-recommendation_amd/csrc/kpp_chain.h and kpp_layout.h.
//
// The chain: k-means++'s prefix sums s_m = fl(s_{m-1} + q_m)
// (initialization.hpp:118-125) as kmeanspp.hip's walk forms them, restated
// serially with the header's functions alone -- per chunk the record if its
// guess holds, else resolve in binades eg / eg + 1 from the prefix arrays with
// one real add at each tie or crossing row, then the rest row by row --
// against the plain loop, EVERY prefix sum bit for bit (NaNs as NaNs). The
// approximate chunk starts the records are built from are sums of q in another
// order than the chain's, as on the device, and deliberately wrong where noted:
// a guess only chooses the path, never the result.
// The layout: lshkm_kpp_shard_ws_bytes is public, so bytes must stay the
// formula callers have sized by; the regions in order, disjoint, aligned.
// Built and run by tests/test_kpp_chain_cpu.py (CPU). Exit code 0 = all equal.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../crypto-recommendation_amd/csrc/kpp_layout.h"

using namespace lshkm;

static int g_bad = 0;
#define EXPECT(c, ...) do { if (!(c)) { g_bad++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

static volatile double g_sink;
static std::vector<double> plain(double s, const std::vector<double>& q) {
    std::vector<double> out(q.size());
    for (size_t i = 0; i < q.size(); i++) { s = s + q[i]; g_sink = s; out[i] = s; }
    return out;
}

// kpp_scan_kernel + kpp_chunk_units_kernel: the approximate starts (start0 +
// the exclusive scan of chunk sums formed per 256-row group, backwards; times
// `scale`: 1, or a deliberate error), then each chunk's record and arrays.
struct Prep {
    std::vector<KppChunk> meta;
    std::vector<int64_t> pa, pb;
};
static Prep prepare(const std::vector<double>& q, double start0, double scale) {
    const int64_t N = (int64_t)q.size(), nch = (N + KPP_CHUNK - 1) / KPP_CHUNK;
    Prep p;
    p.meta.resize(nch);
    p.pa.assign(N, 0);
    p.pb.assign(N, 0);
    std::vector<double> a(nch);
    double run = start0;
    for (int64_t c = 0; c < nch; c++) {
        a[c] = run * scale;
        double cs = 0.0;
        for (int64_t g0 = c * KPP_CHUNK; g0 < N && g0 < (c + 1) * KPP_CHUNK; g0 += KPP_GROUP) {
            double g = 0.0;
            for (int64_t i = std::min<int64_t>(g0 + KPP_GROUP, N) - 1; i >= g0; i--) g += q[i];
            cs += g;
        }
        run += cs;
    }
    for (int64_t c = 0; c < nch; c++) {
        const int64_t r0 = c * KPP_CHUNK, n = std::min<int64_t>(N - r0, KPP_CHUNK);
        const int e = kpp_binade0(a[c]);
        int64_t t = 0;
        int any = 0;
        for (int64_t i = 0; i < n; i++) {
            int cls;
            t += kpp_units(q[r0 + i], e, cls);
            any |= cls;
        }
        const bool has_next = c + 1 < nch;
        p.meta[c] = kpp_chunk_record(a[c], has_next, has_next ? a[c + 1] : 0.0, t, any);
        if (p.meta[c].dual == 0) continue;
        EXPECT(p.meta[c].dual == 2048 + e, "dual names the guessed binade");
        int64_t sa = 0, sb = 0, fa = 0, fb = 0;
        for (int64_t i = 0; i < n; i++) {
            int ca, cb;
            sa += kpp_units(q[r0 + i], e, ca);
            sb += kpp_units(q[r0 + i], e + 1, cb);
            fa += ca == 2;
            fb += cb == 2;
            p.pa[r0 + i] = kpp_entry(sa, fa, ca);
            p.pb[r0 + i] = kpp_entry(sb, fb, cb);
        }
    }
    return p;
}

// kpp_walk (and, for a chunk taken by its record, the rows as kpp_search forms
// them), serially. held: chunks whose guess held.
static std::vector<double> walk(const std::vector<double>& q, const Prep& p, double s, int64_t& held) {
    const int64_t N = (int64_t)q.size(), nch = (int64_t)p.meta.size();
    std::vector<double> out(N);
    held = 0;
    for (int64_t c = 0; c < nch; c++) {
        const int64_t r0 = c * KPP_CHUNK;
        const int n = (int)std::min<int64_t>(N - r0, KPP_CHUNK);
        const KppChunk& m = p.meta[c];
        if (kpp_guess_holds(s, m)) {
            held++;
            const int64_t su = kpp_to_units(s, m.e);
            int64_t run = su;
            for (int i = 0; i < n; i++) {
                int cls;
                run += kpp_units(q[r0 + i], m.e, cls);
                EXPECT(cls == 0, "a chunk taken by its record is clean");
                out[r0 + i] = kpp_from_units(run, m.e);
            }
            s = kpp_from_units(su + m.R, m.e);
            EXPECT(bits(s) == bits(out[r0 + n - 1]), "the record's R is the sum of its rows' units");
            continue;
        }
        int i0 = 0;
        const int eg = m.dual - 2048;
        while (m.dual != 0 && i0 < n) {
            if (!kpp_usable(s)) break;
            const int E = kpp_binade(s);
            if (E != eg && E != eg + 1) break;
            const int64_t* P = (E == eg ? p.pa.data() : p.pb.data()) + r0;
            const int64_t su = kpp_to_units(s, E), base_p = i0 > 0 ? kpp_entry_prefix(P[i0 - 1]) : 0;      // resolve
            int mm = i0;
            for (; mm < n && !kpp_entry_stops(P[mm], su, base_p); mm++)
                out[r0 + mm] = kpp_from_units(su + (kpp_entry_prefix(P[mm]) - base_p), E);
            if (mm > i0) s = out[r0 + mm - 1];
            i0 = mm;
            if (i0 >= n || kpp_entry_poison(P[i0])) break;
            s = s + q[r0 + i0];                       // a tie or crossing row: the real add
            g_sink = s;
            out[r0 + i0++] = s;
        }
        for (int i = i0; i < n; i++) { s = s + q[r0 + i]; g_sink = s; out[r0 + i] = s; }
    }
    return out;
}

// One stream: every prefix sum of the walk against the plain chain. Returns the
// number of chunks whose guess held.
static int64_t run(const char* name, const std::vector<double>& q, double s_in, double scale = 1.0) {
    const std::vector<double> want = plain(s_in, q);
    int64_t held = 0;
    const std::vector<double> got = walk(q, prepare(q, s_in, scale), s_in, held);
    int64_t diff = 0, first = -1;
    for (size_t i = 0; i < q.size(); i++) {
        const bool same = (std::isnan(want[i]) && std::isnan(got[i])) || bits(want[i]) == bits(got[i]);
        if (!same && diff++ == 0) first = (int64_t)i;
    }
    EXPECT(diff == 0, "%s: %lld prefix sums differ, first at row %lld", name, (long long)diff, (long long)first);
    printf("%-28s N %6zu  chunks held %3lld of %3zu  differ %lld\n", name, q.size(), (long long)held,
           (q.size() + KPP_CHUNK - 1) / KPP_CHUNK, (long long)diff);
    return held;
}

static std::vector<double> squares(uint64_t seed, size_t n) {
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<double> q(n);
    for (double& v : q) { const double r = u(g); v = r * r; }
    return q;
}

// Rows of the plain chain whose sum lies in a higher binade than the sum before.
static std::vector<int64_t> crossings(double s_in, const std::vector<double>& q) {
    const std::vector<double> s = plain(s_in, q);
    std::vector<int64_t> rows;
    for (size_t i = 0; i < q.size(); i++) {
        const double before = i ? s[i - 1] : s_in;
        if (before > 0.0 && std::isfinite(s[i]) && std::ilogb(s[i]) > std::ilogb(before)) rows.push_back((int64_t)i);
    }
    return rows;
}

static void check_chain() {
    run("random", squares(1, 20000), 0.0);
    run("random, a shard", squares(2, 5000), 1234.5678);
    {   // ties that round both ways: q / u = 1/2 (the even sum stays) and 9/2 (it moves by 4)
        std::vector<double> m = {1, 1, 1};
        m.insert(m.end(), 600, 0x1p-26);
        m.insert(m.end(), 600, 3 * 0x1p-26);
        m.insert(m.end(), 2, 1.0);
        m.insert(m.end(), 1100, 0x1p-10);
        m.insert(m.end(), 5, 0x1p-27);
        std::vector<double> q(m.size());
        for (size_t i = 0; i < m.size(); i++) q[i] = m[i] * m[i];
        const std::vector<double> s = plain(0.0, q);
        int64_t ties = 0, moved = 0, last_tie = -1;
        for (size_t i = 1; i < q.size(); i++) {
            const double t = std::ldexp(q[i], 52 - std::ilogb(s[i - 1]));      // q in units of the sum before it
            if (t - std::floor(t) == 0.5) { ties++; moved += s[i] != s[i - 1]; last_tie = (int64_t)i; }
        }
        EXPECT(ties == 1200 && moved == 600 && last_tie / KPP_CHUNK == 2, "ties %lld moved %lld last %lld",
               (long long)ties, (long long)moved, (long long)last_tie);
        const std::vector<int64_t> x = crossings(0.0, q);
        EXPECT(x == (std::vector<int64_t>{1, 1203}), "crossings at rows 1 and 1203");
        run("ties both ways", q, 0.0);
    }
    {   // a wrong guess: every chunk falls back, the chain stays exact
        const std::vector<double> q = squares(3, 20000);
        EXPECT(run("starts x 4", q, 100.0, 4.0) == 0, "no guess may hold with every start 4 times too large");
        EXPECT(run("starts x 1/4", q, 100.0, 0.25) == 0, "no guess may hold with every start 4 times too small");
        EXPECT(run("starts right", q, 100.0) > 0, "with the right starts chunks do go by their record");
    }
    {
        std::vector<double> q = squares(4, 3000);
        q[1500] = INFINITY;
        run("one inf row", q, 0.0);
        q[1500] = NAN;
        run("one NaN row", q, 0.0);
    }
    run("zeros", std::vector<double>(1500, 0.0), 0.0);
    {
        std::vector<double> q(2000, 0.0);
        std::fill(q.begin() + 1000, q.end(), 0x1p-60);
        run("zeros, then tiny", q, 0.0);
    }
    {   // two crossings inside one chunk, the first row of them unresolvable in the lower binade
        std::vector<double> q(3000, 0x1p-30);
        q[600] = 1.0;
        q[601] = 2.0;
        const std::vector<int64_t> x = crossings(0.999999, q);
        EXPECT(x.size() >= 2 && x[0] == 600 && x[1] == 601, "rows 600 and 601 each raise the binade");
        run("two crossings in a chunk", q, 0.999999);
    }
    {   // half units at a power of two: absorbed at 2^10; exact ties at 1.0 (an added stream: the sum stays even)
        std::vector<double> q(2048, 1.0);
        std::fill(q.begin() + 1024, q.end(), 0x1p-53);
        run("1024 x 1, 1024 x 2^-53", q, 0.0);
        q.assign(1025, 0x1p-53);
        q[0] = 1.0;
        EXPECT(plain(0.0, q).back() == 1.0, "ties at 1.0 leave it");
        run("1, then ties of 2^-53", q, 0.0);
    }
    {   // a row with q >= 2^(e+1)
        std::vector<double> q = squares(5, 3000);
        q[1500] = 1e9;
        run("one row of 1e9", q, 3.0);
    }
    for (const size_t n : {1, 512, 513, 1537}) {
        run("short, from 0", squares(10 + n, n), 0.0);
        run("short, a shard", squares(20 + n, n), 3.0);
    }
}

static void check_layout_at(int64_t N) {
    const KppLayout w = kpp_layout(N);
    const uint64_t n = (uint64_t)N, nch = (n + 511) / 512, ngroups = (n + 255) / 256;
    const uint64_t parent = 16 * n + 8 * ((ngroups + 1) & ~1ull) + 32 * nch + 4 * ((nch + 1) & ~1ull) + 64 + 8 * 4096 +
                            8 * n + 16 * n;
    EXPECT((uint64_t)w.nch == nch && (uint64_t)w.ngroups == ngroups, "N %lld: counts", (long long)N);
    EXPECT(w.bytes == parent, "N %lld: %zu bytes, the public formula gives %llu", (long long)N, w.bytes,
           (unsigned long long)parent);
    EXPECT(w.dgrid == std::min<uint64_t>(std::max<uint64_t>(ngroups, 1), KPP_DIST_BLOCKS), "N %lld: grid", (long long)N);
    // each region with the bytes its kernels touch, in the order of the map
    const size_t at[] = {w.mind, w.cum, w.gsum, w.cstart, w.meta, w.cs, w.mode, w.mx, w.out, w.bmax, w.qbuf, w.pa, w.pb};
    const uint64_t len[] = {8 * n, 8 * n, 8 * ngroups, 8 * nch, sizeof(KppChunk) * nch, 8 * nch, 4 * nch, 8,
                            sizeof(KppShardOut), 8ull * w.dgrid, 8 * n, 8 * n, 8 * n};
    const int R = (int)(sizeof(at) / sizeof(at[0]));
    EXPECT(at[0] == 0, "N %lld: the first region starts the workspace", (long long)N);
    for (int i = 0; i < R; i++) {
        const uint64_t end = at[i] + len[i], next = i + 1 < R ? at[i + 1] : w.bytes;
        EXPECT(at[i] % 8 == 0 && end <= next, "N %lld: region %d [%zu, %llu) against %llu", (long long)N, i, at[i],
               (unsigned long long)end, (unsigned long long)next);
    }
    EXPECT(w.pb + 8 * n == w.bytes, "N %lld: the last region ends the workspace", (long long)N);
    EXPECT(w.out + sizeof(KppShardOut) <= w.mx + 64 && w.bmax == w.mx + 64, "N %lld: the max word's slot", (long long)N);
}

static void check_layout() {
    static_assert(sizeof(KppChunk) == 16 && sizeof(KppShardOut) == 32, "the records' sizes are part of the formula");
    int64_t count = 0;
    for (int64_t N = 1; N <= 5000; N++, count++) check_layout_at(N);
    for (int64_t M = 256; M <= (1ll << 20); M += 256)
        for (int64_t N = M - 2; N <= M + 2; N++, count++) check_layout_at(N);
    check_layout_at(INT32_MAX);
    printf("layout: %lld sizes\n", (long long)count + 1);
}

int main() {
    check_chain();
    check_layout();
    printf("bad=%d\n", g_bad);
    return g_bad != 0;
}
