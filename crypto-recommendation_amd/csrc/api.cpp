// api.cpp — the C ABI (include/lshkm.h): contexts, handles, parameter
// generation in the reference's RNG draw order, and stream-ordered launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/lshkm.h"
#include "common.h"
#include "kernels.h"
#include "index.h"
#include "kpp_layout.h"

namespace lshkm {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

int device_cu_count(int* ncu) {
    static std::mutex mu;
    static std::map<int, int> cus;             // device index -> CUs
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return kstatus("hipGetDevice");
    std::lock_guard<std::mutex> lock(mu);
    if (!cus.count(dev) &&
        hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        cus.erase(dev);
        return kstatus("hipDeviceGetAttribute");
    }
    *ncu = cus[dev];
    return 0;
}
}  // namespace lshkm

using namespace lshkm;

// ---------------------------------------------------------------- device buffers
namespace lshkm {

Buf::~Buf() { if (p) (void)hipFree(p); }
int Buf::reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    if (hipMalloc(&p, bytes) != hipSuccess) { set_error("hipMalloc failed (" + std::to_string(bytes) + " B)"); p = nullptr; return LSHKM_ERR_NOMEM; }
    cap = bytes;
    return 0;
}

}  // namespace lshkm

extern "C" {

const char* lshkm_last_error(void) { return g_err.c_str(); }
const char* lshkm_version(void) { return "lshkm-gfx950 0.1"; }

int lshkm_ctx_create(int device, lshkm_ctx* out) {
    LSHKM_CHECK(out, LSHKM_ERR_ARG, "out is NULL");
    *out = nullptr;
    // the pow contract (gpow2.h), once per process, before any device work
    if (const int rc = pow_contract_check()) return rc;
    int n = 0;
    LSHKM_HIP(hipGetDeviceCount(&n));
    LSHKM_CHECK(device >= 0 && device < n, LSHKM_ERR_ARG, "device out of range");
    LSHKM_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    LSHKM_HIP(hipGetDeviceProperties(&prop, device));
    LSHKM_CHECK(std::string(prop.gcnArchName).find("gfx950") != std::string::npos, LSHKM_ERR_UNSUPPORTED,
                std::string("liblshkm is built for gfx950 only; device is ") + prop.gcnArchName);
    lshkm_ctx c = new lshkm_ctx_s();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { delete c; set_error("stream create failed"); return LSHKM_ERR_HIP; }
    c->stream = c->own_stream;
    if (c->stats.reserve(sizeof(unsigned long long) * STAT_COUNT)) { delete c; return LSHKM_ERR_NOMEM; }
    (void)hipMemsetAsync(c->stats.p, 0, sizeof(unsigned long long) * STAT_COUNT, c->stream);
    *out = c;
    return 0;
}

int lshkm_ctx_set_stream(lshkm_ctx ctx, void* s) {
    LSHKM_CHECK(ctx, LSHKM_ERR_ARG, "ctx is NULL");
    ctx->stream = (hipStream_t)s;   // verbatim: NULL is the default (null) stream
    return 0;
}

int lshkm_ctx_set_dist_mode(lshkm_ctx ctx, int mode) {
    LSHKM_CHECK(ctx, LSHKM_ERR_ARG, "ctx is NULL");
    LSHKM_CHECK(mode == LSHKM_DIST_CERTIFIED || mode == LSHKM_DIST_EXACT, LSHKM_ERR_ARG,
                "unknown distance mode (LSHKM_DIST_CERTIFIED or LSHKM_DIST_EXACT)");
    ctx->dist_mode = mode;
    return 0;
}

int lshkm_ctx_get_dist_mode(lshkm_ctx ctx, int* mode) {
    LSHKM_CHECK(ctx && mode, LSHKM_ERR_ARG, "bad arguments");
    *mode = ctx->dist_mode;
    return 0;
}

int lshkm_ctx_sync(lshkm_ctx ctx) {
    LSHKM_CHECK(ctx, LSHKM_ERR_ARG, "ctx is NULL");
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int lshkm_dev_alloc(lshkm_ctx ctx, int64_t bytes, void** out) {
    LSHKM_CHECK(ctx && out && bytes >= 0, LSHKM_ERR_ARG, "bad arguments");
    *out = nullptr;
    if (bytes == 0) return 0;
    LSHKM_HIP(hipSetDevice(ctx->device));
    if (hipMalloc(out, (size_t)bytes) != hipSuccess) {
        *out = nullptr;
        set_error("hipMalloc failed (" + std::to_string(bytes) + " B)");
        return LSHKM_ERR_NOMEM;
    }
    return 0;
}

int lshkm_dev_free(lshkm_ctx ctx, void* p) {
    LSHKM_CHECK(ctx, LSHKM_ERR_ARG, "ctx is NULL");
    if (!p) return 0;
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));   // no launch on the stream may still read it
    LSHKM_HIP(hipFree(p));
    return 0;
}

int lshkm_memcpy_h2d(lshkm_ctx ctx, void* dst_dev, const void* src_host, int64_t bytes) {
    LSHKM_CHECK(ctx && bytes >= 0 && (bytes == 0 || (dst_dev && src_host)), LSHKM_ERR_ARG, "bad arguments");
    if (bytes == 0) return 0;
    LSHKM_HIP(hipMemcpyAsync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));   // the host buffer may be reused on return
    return 0;
}

int lshkm_memcpy_d2h(lshkm_ctx ctx, void* dst_host, const void* src_dev, int64_t bytes) {
    LSHKM_CHECK(ctx && bytes >= 0 && (bytes == 0 || (dst_host && src_dev)), LSHKM_ERR_ARG, "bad arguments");
    if (bytes == 0) return 0;
    LSHKM_HIP(hipMemcpyAsync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int lshkm_ctx_destroy(lshkm_ctx ctx) {
    if (!ctx) return 0;
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return 0;
}

int lshkm_get_stat(lshkm_ctx ctx, int which, int64_t* v) {
    LSHKM_CHECK(ctx && v && which >= 0 && which < STAT_COUNT, LSHKM_ERR_ARG, "bad stat query");
    unsigned long long x = 0;
    LSHKM_HIP(hipMemcpyAsync(&x, (unsigned long long*)ctx->stats.p + which, sizeof(x), hipMemcpyDeviceToHost, ctx->stream));
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));
    *v = (int64_t)x;
    return 0;
}

int lshkm_ctx_enable_timing(lshkm_ctx ctx, int on) {
    LSHKM_CHECK(ctx, LSHKM_ERR_ARG, "ctx is NULL");
    for (hipEvent_t& e : ctx->tev)
        if (!e) LSHKM_HIP(hipEventCreate(&e));
    ctx->timing = on != 0;
    return 0;
}

// The fused pass: from before the prep to the later of the main stream's last
// fused launch and the side stream's hash fix-up.
int lshkm_last_kernel_ms(lshkm_ctx ctx, float* ms) {
    LSHKM_CHECK(ctx && ms && ctx->tev[1], LSHKM_ERR_STATE, "timing not enabled");
    LSHKM_HIP(hipEventSynchronize(ctx->tev[1]));
    LSHKM_HIP(hipEventElapsedTime(ms, ctx->tev[0], ctx->tev[1]));
    if (ctx->tev_side) {
        float m2 = 0.f;
        LSHKM_HIP(hipEventSynchronize(ctx->tev[2]));
        LSHKM_HIP(hipEventElapsedTime(&m2, ctx->tev[0], ctx->tev[2]));
        *ms = std::max(*ms, m2);
    }
    return 0;
}

int lshkm_reset_stats(lshkm_ctx ctx) {
    LSHKM_CHECK(ctx, LSHKM_ERR_ARG, "ctx is NULL");
    LSHKM_HIP(hipMemsetAsync(ctx->stats.p, 0, sizeof(unsigned long long) * STAT_COUNT, ctx->stream));
    return 0;
}

// ------------------------------------------------------------ parameter generation
// The reference's generators draw from one std::default_random_engine seeded
// with the clock (lsh_cube.hpp:49-51); each EuclideanHGen owns a fresh
// normal_distribution<float> (euclidean_h_gen.hpp:58) so an odd d drops the
// cached second variate; CosineHGen likewise with double (cosine_h_gen.hpp:54).
static uint32_t engine_state(std::default_random_engine& g) {
    std::ostringstream os;
    os << g;
    return (uint32_t)std::stoul(os.str());
}

static void draw_euclid_h(std::default_random_engine& g, int d, float w, float* v, float* t) {
    std::normal_distribution<float> nd(0, 1);
    for (int j = 0; j < d; j++) v[j] = nd(g);
    std::uniform_real_distribution<float> ud(0, w);
    *t = ud(g);
}

static void draw_cosine_h(std::default_random_engine& g, int d, double* r) {
    std::normal_distribution<double> nd(0, 1);
    for (int j = 0; j < d; j++) r[j] = nd(g);
}

int lshkm_params_lsh_euclidean(uint64_t seed, int L, int k, int d, float w, float* V, float* t, int32_t* r,
                               uint32_t* state) {
    LSHKM_CHECK(L > 0 && k > 0 && d > 0 && V && t && r, LSHKM_ERR_ARG, "bad arguments");
    std::default_random_engine g;
    g.seed((unsigned long)seed);
    for (int l = 0; l < L; l++) {
        std::uniform_int_distribution<int> uid(0, 100);   // euclidean_phi_gen.hpp:63
        for (int i = 0; i < k; i++) {
            const size_t li = (size_t)l * k + i;
            draw_euclid_h(g, d, w, V + li * d, t + li);
            r[li] = uid(g);
        }
    }
    if (state) *state = engine_state(g);
    return 0;
}

int lshkm_params_lsh_cosine(uint64_t seed, int L, int k, int d, double* R, uint32_t* state) {
    LSHKM_CHECK(L > 0 && k > 0 && d > 0 && R, LSHKM_ERR_ARG, "bad arguments");
    std::default_random_engine g;
    g.seed((unsigned long)seed);
    for (int l = 0; l < L; l++)
        for (int i = 0; i < k; i++) draw_cosine_h(g, d, R + ((size_t)l * k + i) * d);
    if (state) *state = engine_state(g);
    return 0;
}

int lshkm_params_cube_euclidean(uint64_t seed, int k, int d, float w, float* V, float* t, uint32_t* state) {
    LSHKM_CHECK(k > 0 && d > 0 && V && t, LSHKM_ERR_ARG, "bad arguments");
    std::default_random_engine g;
    g.seed((unsigned long)seed);
    for (int i = 0; i < k; i++) draw_euclid_h(g, d, w, V + (size_t)i * d, t + i);
    if (state) *state = engine_state(g);
    return 0;
}

// EuclideanF coins on the host (sharded builds): per entry in order,
// c = uniform_int_distribution<int>(1, 2) over the shared minstd_rand0
// (euclidean_f_gen.hpp:68-76), bit = mod(h, c) (utils.hpp:97-98). libstdc++'s
// own engine and distribution, resumed from the engine state value.
int lshkm_coins_draw(uint32_t* rng_state, const int32_t* h, int64_t n, int32_t* bit) {
    LSHKM_CHECK(rng_state && n >= 0 && (n == 0 || (h && bit)), LSHKM_ERR_ARG, "bad arguments");
    std::default_random_engine g;
    g.seed((unsigned long)*rng_state);
    LSHKM_CHECK(engine_state(g) == *rng_state, LSHKM_ERR_ARG, "rng_state is not a minstd_rand0 state");
    for (int64_t i = 0; i < n; i++) {
        std::uniform_int_distribution<int> coin(1, 2);
        const int c = coin(g);
        bit[i] = (h[i] % c + c) % c;
    }
    *rng_state = engine_state(g);
    return 0;
}

int lshkm_rand_selection(uint64_t seed, int64_t N, int K, int32_t* rows) {
    LSHKM_CHECK(rows && N >= 1 && N <= INT32_MAX && K >= 1 && K <= N, LSHKM_ERR_ARG,
                "bad arguments (need 1 <= K <= N < 2^31)");
    std::default_random_engine g;
    g.seed((unsigned long)seed);
    std::uniform_int_distribution<int> uni(0, (int)(N - 1));
    rows[0] = uni(g);
    for (int i = 1; i < K; i++) {
        int r = uni(g), c = 0;
        while (c < i) {          // redraw on a repeat and check all again (initialization.hpp:53-61)
            if (rows[c] == r) { r = uni(g); c = 0; }
            else c++;
        }
        rows[i] = r;
    }
    return 0;
}

// Every engine draw of k_means_pp up front (initialization.hpp:75-79,132-133):
// they do not depend on the data. uniform_real<double>(0, total) is
// canon * (total - 0) + 0 with canon = uniform_real<double>(0, 1).
int lshkm_kpp_draws(uint64_t seed, int64_t N_total, int K, int64_t* first_row, double* canon) {
    LSHKM_CHECK(first_row && canon && N_total >= 1 && N_total <= INT32_MAX && K >= 1, LSHKM_ERR_ARG,
                "bad arguments (need 1 <= N < 2^31, K >= 1)");
    std::default_random_engine g;
    g.seed((unsigned long)seed);
    std::uniform_int_distribution<int> uni(0, (int)(N_total - 1));
    *first_row = uni(g);
    canon[0] = 0.0;
    for (int i = 1; i < K; i++) {
        std::uniform_real_distribution<double> unit(0.0, 1.0);
        canon[i] = unit(g);
    }
    return 0;
}

}  // extern "C"

static int kmeans_pp_impl(lshkm_ctx ctx, Pts X, int64_t N, int d, int K, int metric, uint64_t seed, int32_t* rows) {
    LSHKM_CHECK(ctx && X.p && rows && N >= 1 && N <= INT32_MAX && d >= 1 && d <= 4096 && K >= 1, LSHKM_ERR_ARG,
                "bad arguments (need N < 2^31, 1 <= d <= 4096, K >= 1)");
    LSHKM_CHECK(metric == LSHKM_METRIC_EUCLIDEAN || metric == LSHKM_METRIC_COSINE, LSHKM_ERR_ARG, "unknown metric");
    LSHKM_HIP(hipSetDevice(ctx->device));
    std::vector<int32_t> chosen(K, 0);
    std::vector<double> canon(K, 0.0);
    int64_t first = 0;
    if (const int rc = lshkm_kpp_draws(seed, N, K, &first, canon.data())) return rc;
    chosen[0] = (int32_t)first;
    Buf &ws = ctx->ws_call[0], &dch = ctx->ws_call[1], &dcanon = ctx->ws_call[2];
    int rc;
    if ((rc = ws.reserve(kpp_layout(N).bytes)) || (rc = dch.reserve(sizeof(int32_t) * K)) ||
        (rc = dcanon.reserve(sizeof(double) * K)))
        return rc;
    LSHKM_HIP(hipMemcpyAsync(dch.p, chosen.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, ctx->stream));
    LSHKM_HIP(hipMemcpyAsync(dcanon.p, canon.data(), sizeof(double) * K, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_kmeans_pp(ctx->stream, X, N, d, K, metric, dcanon.as<double>(), dch.as<int32_t>(), ws.p,
                               (unsigned long long*)ctx->stats.p))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    LSHKM_HIP(hipMemcpyAsync(rows, dch.p, sizeof(int32_t) * K, hipMemcpyDeviceToHost, ctx->stream));
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" {

int lshkm_kmeans_pp(lshkm_ctx ctx, const float* X, int64_t N, int d, int K, int metric, uint64_t seed,
                    int32_t* rows) {
    return kmeans_pp_impl(ctx, X, N, d, K, metric, seed, rows);
}

int lshkm_kmeans_pp_f64(lshkm_ctx ctx, const double* X, int64_t N, int d, int K, int metric, uint64_t seed,
                        int32_t* rows) {
    return kmeans_pp_impl(ctx, X, N, d, K, metric, seed, rows);
}

}  // extern "C"

// k_means_pp over row shards (lshkm_kpp_shard_*): one step of one iteration on
// this rank's n rows; an empty shard touches no memory. `out` is what the step
// leaves for the host behind the workspace's max word (kpp_layout.h).
static int kpp_shard_ws_check(lshkm_ctx ctx, int64_t n, const void* ws, int64_t ws_bytes) {
    LSHKM_CHECK(ctx && n >= 0 && n <= INT32_MAX, LSHKM_ERR_ARG, "bad arguments (need 0 <= n < 2^31)");
    LSHKM_CHECK(n == 0 || (ws && ws_bytes >= 0 && (size_t)ws_bytes >= kpp_layout(n).bytes), LSHKM_ERR_ARG,
                "workspace smaller than lshkm_kpp_shard_ws_bytes");
    LSHKM_HIP(hipSetDevice(ctx->device));
    return 0;
}

static int kpp_shard_read(lshkm_ctx ctx, int64_t n, const void* ws, int launch_rc, KppShardOut* out) {
    if (launch_rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return launch_rc;
    }
    LSHKM_HIP(hipMemcpyAsync(out, (const char*)ws + kpp_layout(n).out, sizeof(*out), hipMemcpyDeviceToHost,
                             ctx->stream));
    LSHKM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

static int kpp_shard_dist_impl(lshkm_ctx ctx, Pts X, int64_t n, int d, int metric, const void* c, int it, void* ws,
                               int64_t ws_bytes, uint64_t* max_bits, double* sum) {
    if (const int rc = kpp_shard_ws_check(ctx, n, ws, ws_bytes)) return rc;
    LSHKM_CHECK(max_bits && sum && d >= 1 && d <= 4096 && it >= 1, LSHKM_ERR_ARG,
                "bad arguments (need 1 <= d <= 4096, it >= 1)");
    LSHKM_CHECK(metric == LSHKM_METRIC_EUCLIDEAN || metric == LSHKM_METRIC_COSINE, LSHKM_ERR_ARG, "unknown metric");
    *max_bits = 0;
    *sum = 0.0;
    if (n == 0) return 0;
    LSHKM_CHECK(X.p && c, LSHKM_ERR_ARG, "rows or centroid row is NULL");
    KppShardOut o;
    const int lrc = launch_kpp_shard_dist(ctx->stream, X, n, d, metric, c, it, ws);
    if (const int rc = kpp_shard_read(ctx, n, ws, lrc, &o)) return rc;
    *max_bits = o.max_bits;
    *sum = o.sum;
    return 0;
}

extern "C" {

int lshkm_kpp_shard_ws_bytes(int64_t n, int64_t* bytes) {
    LSHKM_CHECK(bytes && n >= 0 && n <= INT32_MAX, LSHKM_ERR_ARG, "bad arguments (need 0 <= n < 2^31)");
    *bytes = (int64_t)kpp_layout(n).bytes;
    return 0;
}

int lshkm_kpp_shard_dist(lshkm_ctx ctx, const float* X, int64_t n, int d, int metric, const float* c, int it, void* ws,
                         int64_t ws_bytes, uint64_t* max_bits, double* sum) {
    return kpp_shard_dist_impl(ctx, X, n, d, metric, c, it, ws, ws_bytes, max_bits, sum);
}

int lshkm_kpp_shard_dist_f64(lshkm_ctx ctx, const double* X, int64_t n, int d, int metric, const double* c, int it,
                             void* ws, int64_t ws_bytes, uint64_t* max_bits, double* sum) {
    return kpp_shard_dist_impl(ctx, X, n, d, metric, c, it, ws, ws_bytes, max_bits, sum);
}

int lshkm_kpp_shard_units(lshkm_ctx ctx, int64_t n, uint64_t gmax_bits, double start, void* ws, int64_t ws_bytes) {
    if (const int rc = kpp_shard_ws_check(ctx, n, ws, ws_bytes)) return rc;
    if (n == 0) return 0;
    return launch_kpp_shard_units(ctx->stream, n, gmax_bits, start, ws);
}

int lshkm_kpp_shard_chain(lshkm_ctx ctx, int64_t n, double s_in, void* ws, int64_t ws_bytes, double* s_out) {
    if (const int rc = kpp_shard_ws_check(ctx, n, ws, ws_bytes)) return rc;
    LSHKM_CHECK(s_out, LSHKM_ERR_ARG, "s_out is NULL");
    *s_out = s_in;
    if (n == 0) return 0;
    KppShardOut o;
    const int lrc = launch_kpp_shard_chain(ctx->stream, n, s_in, ws, (unsigned long long*)ctx->stats.p);
    if (const int rc = kpp_shard_read(ctx, n, ws, lrc, &o)) return rc;
    *s_out = o.s_out;
    return 0;
}

int lshkm_kpp_shard_pick(lshkm_ctx ctx, int64_t n, double rd, int owns_row0, void* ws, int64_t ws_bytes,
                         int64_t* row) {
    if (const int rc = kpp_shard_ws_check(ctx, n, ws, ws_bytes)) return rc;
    LSHKM_CHECK(row, LSHKM_ERR_ARG, "row is NULL");
    *row = -1;
    if (n == 0) return 0;
    KppShardOut o;
    const int lrc = launch_kpp_shard_pick(ctx->stream, n, rd, owns_row0, ws);
    if (const int rc = kpp_shard_read(ctx, n, ws, lrc, &o)) return rc;
    LSHKM_CHECK(o.pick >= -1 && o.pick < n, LSHKM_ERR_STATE, "pick outside the shard (rd above the running sum?)");
    *row = o.pick;
    return 0;
}

int lshkm_params_cube_cosine(uint64_t seed, int k, int d, double* R, uint32_t* state) {
    LSHKM_CHECK(k > 0 && d > 0 && R, LSHKM_ERR_ARG, "bad arguments");
    std::default_random_engine g;
    g.seed((unsigned long)seed);
    for (int i = 0; i < k; i++) draw_cosine_h(g, d, R + (size_t)i * d);
    if (state) *state = engine_state(g);
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------ projection tables
namespace lshkm {

int ProjTable::upload(hipStream_t s, int metric_, int d_, int L_, int k_, float w_, const float* V, const float* t,
                      const int32_t* r, const double* R) {
    metric = metric_; d = d_; L = L_; k = k_; w = w_;
    LK = L * k;
    LKpad = hash_lkpad(LK);
    const int drows = (d + 3) / 4 * 4;    // zero pad rows: the kernel reads x in float4 steps
    std::vector<double> PT((size_t)drows * LKpad, 0.0), pn(LK, 0.0);
    std::vector<float> tt(LK, 0.f);
    std::vector<int32_t> rr(LK, 0);
    for (int f = 0; f < LK; f++) {
        long double n2 = 0.0L;
        for (int j = 0; j < d; j++) {
            const double v = metric == LSHKM_METRIC_EUCLIDEAN ? (double)V[(size_t)f * d + j] : R[(size_t)f * d + j];
            PT[(size_t)j * LKpad + f] = v;
            n2 += (long double)v * (long double)v;
        }
        pn[f] = (double)sqrtl(n2) * (1.0 + 0x1p-40);
        if (metric == LSHKM_METRIC_EUCLIDEAN) { tt[f] = t ? t[f] : 0.f; rr[f] = r ? r[f] : 0; }
    }
    int rc;
    if ((rc = PT_d.reserve(PT.size() * 8)) || (rc = t_d.reserve(LK * 4)) || (rc = pn_d.reserve(LK * 8)) ||
        (rc = r_d.reserve(LK * 4)))
        return rc;
    LSHKM_HIP(hipMemcpyAsync(PT_d.p, PT.data(), PT.size() * 8, hipMemcpyHostToDevice, s));
    LSHKM_HIP(hipMemcpyAsync(t_d.p, tt.data(), LK * 4, hipMemcpyHostToDevice, s));
    LSHKM_HIP(hipMemcpyAsync(pn_d.p, pn.data(), LK * 8, hipMemcpyHostToDevice, s));
    LSHKM_HIP(hipMemcpyAsync(r_d.p, rr.data(), LK * 4, hipMemcpyHostToDevice, s));
    // split-f16 image for the fused hash+assign kernel (euclidean) and the
    // MFMA hash (either metric; cosine splits the fp64 rows of R)
    // the fused kernels' phi arithmetic assumes the reference's r range
    // [0, 100] (euclidean_phi_gen.hpp:64; tile.h phi_term_small)
    bool r_small = true;
    for (int f = 0; f < LK; f++) r_small = r_small && rr[f] >= 0 && rr[f] <= 100;
    fused_ok = metric == LSHKM_METRIC_EUCLIDEAN && d == 128 && LK <= 32 && r_small;
    mfma_ok = d == 128 && LK <= 32;
    std::vector<_Float16> vh, vl;
    std::vector<double> v1;
    if (mfma_ok) {
        vh.assign(64 * 128, (_Float16)0.f);
        vl.assign(64 * 128, (_Float16)0.f);
        v1.assign(LK, 0.0);
        for (int f = 0; f < LK; f++) {
            long double s1 = 0.0L;
            for (int j = 0; j < 128; j++) {
                const double v = metric == LSHKM_METRIC_EUCLIDEAN ? (double)V[(size_t)f * d + j] : R[(size_t)f * d + j];
                const _Float16 hv = (_Float16)v;
                vh[f * 128 + j] = hv;
                vl[f * 128 + j] = (_Float16)(float)(v - (double)hv);   // v - hv is exact in fp64
                s1 += fabsl((long double)v);
            }
            v1[f] = (double)s1 * (1.0 + 0x1p-40);
        }
        if ((rc = vh_d.reserve(vh.size() * 2)) || (rc = vl_d.reserve(vl.size() * 2)) || (rc = v1_d.reserve(LK * 8)))
            return rc;
        LSHKM_HIP(hipMemcpyAsync(vh_d.p, vh.data(), vh.size() * 2, hipMemcpyHostToDevice, s));
        LSHKM_HIP(hipMemcpyAsync(vl_d.p, vl.data(), vl.size() * 2, hipMemcpyHostToDevice, s));
        LSHKM_HIP(hipMemcpyAsync(v1_d.p, v1.data(), LK * 8, hipMemcpyHostToDevice, s));
    }
    LSHKM_HIP(hipStreamSynchronize(s));   // host vectors go out of scope
    // host copies kept for introspection
    hV.assign(V ? V : (const float*)nullptr, V ? V + (size_t)LK * d : nullptr);
    return 0;
}

HashParams ProjTable::params(int64_t nb) const {
    HashParams p;
    p.PT = (const double*)PT_d.p;
    p.t = (const float*)t_d.p;
    p.pnorm = (const double*)pn_d.p;
    p.r = (const int32_t*)r_d.p;
    p.w = w;
    p.d = d; p.L = L; p.k = k; p.LK = LK; p.LKpad = LKpad;
    p.nb = nb;
    return p;
}

HashMfmaParams ProjTable::mfma_params(int64_t nb) const {
    HashMfmaParams p;
    p.Vh = vh_d.as<_Float16>(); p.Vl = vl_d.as<_Float16>();
    p.t = (const float*)t_d.p; p.pnorm = (const double*)pn_d.p; p.v1 = (const double*)v1_d.p;
    p.r = (const int32_t*)r_d.p; p.PT = (const double*)PT_d.p;
    p.w = w;
    p.d = d; p.L = L; p.k = k; p.LK = LK; p.LKpad = LKpad;
    p.nb = nb;
    return p;
}

}  // namespace lshkm

extern "C" {

// ----------------------------------------------------------------------- LSH
int lshkm_lsh_create(lshkm_ctx ctx, int metric, int d, int k, int L, int64_t nb, float w, const float* V,
                     const float* t, const int32_t* r, const double* R, lshkm_lsh* out) {
    LSHKM_CHECK(ctx && out, LSHKM_ERR_ARG, "ctx/out is NULL");
    LSHKM_CHECK(d > 0 && d <= 1024 && k > 0 && L > 0 && L * k <= 256, LSHKM_ERR_ARG, "unsupported d/k/L");
    LSHKM_CHECK(k <= 30, LSHKM_ERR_ARG, "k > 30");
    if (metric == LSHKM_METRIC_EUCLIDEAN) {
        LSHKM_CHECK(V && t && r, LSHKM_ERR_ARG, "euclidean LSH needs V, t, r");
        LSHKM_CHECK(nb > 0 && nb < (1ll << 31), LSHKM_ERR_ARG, "nb must be in [1, 2^31)");   // mod by 0 crashes the reference
        LSHKM_CHECK(w > 0.f, LSHKM_ERR_ARG, "w must be > 0");
    } else if (metric == LSHKM_METRIC_COSINE) {
        LSHKM_CHECK(R, LSHKM_ERR_ARG, "cosine LSH needs R");
        nb = (int64_t)1 << k;
    } else {
        set_error("unknown metric");
        return LSHKM_ERR_ARG;
    }
    LSHKM_HIP(hipSetDevice(ctx->device));
    lshkm_lsh h = new lshkm_lsh_s();
    h->ctx = ctx; h->metric = metric; h->nb = nb;
    int rc = h->proj.upload(ctx->stream, metric, d, L, k, w, V, t, r, R);
    if (rc) { delete h; return rc; }
    *out = h;
    return 0;
}

int lshkm_lsh_destroy(lshkm_lsh lsh) {
    if (!lsh) return 0;
    (void)hipDeviceSynchronize();   // never touches lsh->ctx: it may already be destroyed
    delete lsh;
    return 0;
}

}  // extern "C"

static int lsh_hash_impl(lshkm_lsh lsh, Pts X, int64_t N, int32_t* tuples, int32_t* phi, int32_t* bucket) {
    LSHKM_CHECK(lsh && (X.p || N == 0) && N >= 0, LSHKM_ERR_ARG, "bad arguments");
    lshkm_ctx ctx = lsh->ctx;
    LSHKM_HIP(hipSetDevice(ctx->device));
    const int mode = lsh->metric == LSHKM_METRIC_EUCLIDEAN ? HM_LSH_EUCLID : HM_LSH_COSINE;
    const int rc = hash_rows(ctx, mode, X, N, lsh->proj, lsh->nb, mode == HM_LSH_EUCLID ? tuples : nullptr, phi, bucket,
                             nullptr);
    if (rc) { LSHKM_LAUNCH_CHECK(); return rc; }
    return 0;
}

extern "C" {

int lshkm_lsh_hash(lshkm_lsh lsh, const float* X, int64_t N, int32_t* tuples, int32_t* phi, int32_t* bucket) {
    return lsh_hash_impl(lsh, X, N, tuples, phi, bucket);
}

int lshkm_lsh_hash_f64(lshkm_lsh lsh, const double* X, int64_t N, int32_t* tuples, int32_t* phi, int32_t* bucket) {
    return lsh_hash_impl(lsh, X, N, tuples, phi, bucket);
}

// ------------------------------------------------------------------- Lloyd
}  // extern "C"

// Kernel path for assignment: the split-f16 fused pass where one of its forms
// runs the shape (fused_route, fused_layout.h: fp32 rows of d = 128 -- path 0
// -- and, K <= 512, fp64 rows and fp32 rows of d < 128 zero-padded dims -- path
// 3), else the f32-MFMA kernel (d <= 256; fp64 rows rounded to f32 on load, the
// bound widened accordingly), else the exact pass.
// LSHKM_ASSIGN_PATH = "f32" / "exact" forces a path (tests compare them).
static int assign_path(int metric, int d, int K, bool f64) {
    if (test_switch("LSHKM_ASSIGN_PATH", "exact")) return 2;
    if (!test_switch("LSHKM_ASSIGN_PATH", "f32")) {
        const FusedRoute r = fused_route(metric != LSHKM_METRIC_EUCLIDEAN, f64, d, K, false, 0, 0,
                                         test_switch("LSHKM_FUSED_FORM", "chunked"));
        if (r.form != FusedForm::none) return r.rows == 0 ? 0 : 3;
    }
    return assign_dp(d) > 0 ? 1 : 2;
}

// One pass for hashing + assignment: an index of the assignment's metric whose
// split image is on the device (euclidean: fused_ok, r within the fix-up's
// range), on the shapes a fused form hashes (fused_route: L*k <= 32; cosine k = 4)
static bool fuse_hash(const lshkm_lsh_s* lsh, int metric, int K, bool f64) {
    const lshkm::ProjTable& pj = lsh->proj;
    if (lsh->metric != metric || !(metric == LSHKM_METRIC_EUCLIDEAN ? pj.fused_ok : pj.mfma_ok)) return false;
    return fused_route(metric != LSHKM_METRIC_EUCLIDEAN, f64, pj.d, K, true, pj.k, pj.LK,
                       test_switch("LSHKM_FUSED_FORM", "chunked")).form != FusedForm::none;
}

// The exact pass's form (exact_route, exact_layout.h); LSHKM_EXACT_PASS=full:
// no pruning
ExactForm lshkm::exact_form(const AssignJob& q) {
    return exact_route(q.metric != LSHKM_METRIC_EUCLIDEAN, q.X.f64, q.d, q.K, test_switch("LSHKM_EXACT_PASS", "full"));
}

int lshkm::exact_listed_prep(lshkm_ctx ctx, const AssignJob& q) {
    const ExactForm form = exact_form(q);
    int rc;
    if ((rc = ctx->ws_ct.reserve(exact_ws_bytes(form, q.d, q.K)))) return rc;
    return launch_exact_prep(ctx->stream, q, form, ctx->ws_ct.p);
}

int lshkm::exact_listed(lshkm_ctx ctx, const AssignJob& q, const RowList& l, bool exact_dist, bool prepped,
                        const double* xn2, const double* nbv) {
    int rc;
    if (!prepped && l.bound > 0 && (rc = exact_listed_prep(ctx, q))) return rc;
    return launch_exact_pass(ctx->stream, q, l, exact_form(q), ctx->ws_ct.p, exact_dist, xn2, nbv);
}

// The f32-MFMA sequence (d <= 256): certified scores, the listed exact pass,
// the cosine distance fix-ups.
static int assign_f32_mfma(lshkm_ctx ctx, const AssignJob& q) {
    hipStream_t s = ctx->stream;
    const int DP = assign_dp(q.d), Kpad = (q.K + 63) / 64 * 64;
    const int64_t N = q.N;
    int rc;
    if ((rc = ctx->ws_c32.reserve((size_t)Kpad * DP * 4)) || (rc = ctx->ws_cconst.reserve((size_t)3 * Kpad * 4)) ||
        (rc = ctx->ws_ambig.reserve((size_t)std::max<int64_t>(N, 1) * 2 * 4)) ||   // ambiguous rows | cosine fix-ups
        (rc = ctx->ws_counter.reserve(64)))
        return rc;
    unsigned long long* cnt = (unsigned long long*)ctx->ws_counter.p;
    ctx->ws_dirty();              // ws_counter / ws_cconst: not as fused_assign left them
    LSHKM_HIP(hipMemsetAsync(cnt, 0, 16, s));
    if ((rc = launch_centroid_prep(s, q.C, q.K, Kpad, q.d, DP, q.metric, q.X.f64, (float*)ctx->ws_c32.p, (float*)ctx->ws_cconst.p))) return rc;
    if ((rc = launch_assign_mfma(s, q.X, N, q.d, DP, q.C, q.K, Kpad, q.metric, (const float*)ctx->ws_c32.p, (const float*)ctx->ws_cconst.p,
                                 q.assign, q.dist, (int32_t*)ctx->ws_ambig.p, cnt))) return rc;
    RowList l;
    l.p = (int32_t*)ctx->ws_ambig.p; l.count = cnt; l.bound = N;
    if ((rc = exact_listed(ctx, q, l, true, false, nullptr, nullptr))) return rc;
    if (q.metric != LSHKM_METRIC_EUCLIDEAN &&
        ((rc = launch_cos_fix(s, q.X, N, q.d, q.C, (const int32_t*)ctx->ws_ambig.p + N, cnt + 1, q.assign, q.dist)) ||
         (rc = launch_add_counter(s, (unsigned long long*)ctx->stats.p + STAT_COS_FIX, cnt + 1)))) return rc;
    // ambiguous-count statistic
    return launch_add_counter(s, (unsigned long long*)ctx->stats.p + STAT_ASSIGN_AMBIG, cnt);
}

// The centroid override's source rows into ws_src on the context's stream.
static int stage_override(lshkm_ctx ctx, const int32_t* src_rows_host, int K) {
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = ctx->ws_src.reserve((size_t)K * 4))) return rc;
    // The same rows as the previous override already sit in ws_src (Lloyd
    // iterations and the bench pass one array repeatedly): no copy. A small
    // host->device copy blocked the host until the stream drained, so every
    // call waited for the previous one's tail: 2.05 ms of host enqueue per call vs 0.05).
    const bool same = ctx->src_cache_dev == ctx->ws_src.p && ctx->src_cache_cap == ctx->ws_src.cap &&
                      ctx->src_cache.size() == (size_t)K &&
                      std::memcmp(ctx->src_cache.data(), src_rows_host, (size_t)K * 4) == 0;
    if (same) return 0;
    // Stage through a pinned buffer so the caller's array may be freed at
    // once and no stream sync is needed (a ring of buffers, index.h).
    if ((rc = ctx->pin_stage((size_t)K * 4))) return rc;
    std::memcpy(ctx->pinned, src_rows_host, (size_t)K * 4);
    LSHKM_HIP(hipMemcpyAsync(ctx->ws_src.p, ctx->pinned, (size_t)K * 4, hipMemcpyHostToDevice, s));
    LSHKM_HIP(hipEventRecord(ctx->pinned_ev, s));
    ctx->src_cache.assign(src_rows_host, src_rows_host + K);
    ctx->src_cache_dev = ctx->ws_src.p;
    ctx->src_cache_cap = ctx->ws_src.cap;
    return 0;
}

// force_exact: exact distances whatever the context's mode (range
// assignment's leftover rows: a range assignment is exact-order in either mode)
static int assign_impl(lshkm_ctx ctx, Pts X, int64_t N, int d, const double* C, int K, int metric,
                       const int32_t* src_rows_host, int32_t* assign, double* dist, lshkm_lsh lsh, int32_t* tuples,
                       int32_t* phi, int32_t* bucket, bool force_exact = false) {
    hipStream_t s = ctx->stream;
    const int path = assign_path(metric, d, K, X.f64);
    AssignRequest q;
    q.X = X; q.N = N; q.d = d; q.C = C; q.K = K; q.metric = metric; q.assign = assign; q.dist = dist;
    q.tuples = tuples; q.phi = phi; q.bucket = bucket; q.force_exact = force_exact;
    if (lsh && path == 0 && fuse_hash(lsh, metric, K, X.f64)) q.lsh = lsh;
    int rc;
    if (lsh && !q.lsh && (rc = hash_rows(ctx, lsh->metric == LSHKM_METRIC_EUCLIDEAN ? HM_LSH_EUCLID : HM_LSH_COSINE,
                                         X, N, lsh->proj, lsh->nb,
                                         lsh->metric == LSHKM_METRIC_EUCLIDEAN ? tuples : nullptr, phi, bucket,
                                         nullptr))) { LSHKM_LAUNCH_CHECK(); return rc; }
    const bool fused = path == 0 || path == 3;
    // the centroid override: staged ahead of a fused pass, whose last kernel
    // applies it; a launch of its own after the other paths
    if (src_rows_host && (rc = stage_override(ctx, src_rows_host, K))) return rc;
    if (fused) {
        if (src_rows_host) q.src_dev = (const int32_t*)ctx->ws_src.p;
        rc = fused_assign(ctx, q);
    } else if (path == 1) rc = assign_f32_mfma(ctx, q);
    else {
        // Exact reference-order pass over every centroid (cosine metric, or d > 256).
        RowList all;
        all.bound = N;
        rc = launch_exact_pass(s, q, all, ExactForm::every, nullptr, true, nullptr, nullptr);
    }
    if (rc) { LSHKM_LAUNCH_CHECK(); return rc; }
    if (src_rows_host && !fused &&
        (rc = launch_assign_override(s, (const int32_t*)ctx->ws_src.p, K, N, assign, dist))) { LSHKM_LAUNCH_CHECK(); return rc; }
    return 0;
}

static int lloyd_impl(lshkm_ctx ctx, Pts X, int64_t N, int d, const double* C, int K, int metric,
                      const int32_t* src_rows_host, int32_t* assign, double* dist) {
    LSHKM_CHECK(ctx && (X.p || N == 0) && C && (assign || N == 0) && (dist || N == 0) && N >= 0 && d > 0 && K > 0,
                LSHKM_ERR_ARG, "bad arguments");
    LSHKM_CHECK(metric == LSHKM_METRIC_EUCLIDEAN || metric == LSHKM_METRIC_COSINE, LSHKM_ERR_ARG, "unknown metric");
    LSHKM_HIP(hipSetDevice(ctx->device));
    return assign_impl(ctx, X, N, d, C, K, metric, src_rows_host, assign, dist, nullptr, nullptr, nullptr, nullptr);
}

static int hash_assign_impl(lshkm_lsh lsh, Pts X, int64_t N, const double* C, int K, const int32_t* src_rows_host,
                            int32_t* tuples, int32_t* phi, int32_t* bucket, int32_t* assign, double* dist,
                            int metric = LSHKM_METRIC_EUCLIDEAN) {
    LSHKM_CHECK(lsh && (X.p || N == 0) && C && (assign || N == 0) && (dist || N == 0) && N >= 0 && K > 0, LSHKM_ERR_ARG,
                "bad arguments");
    lshkm_ctx ctx = lsh->ctx;
    LSHKM_HIP(hipSetDevice(ctx->device));
    LSHKM_CHECK(metric == LSHKM_METRIC_EUCLIDEAN || metric == LSHKM_METRIC_COSINE, LSHKM_ERR_ARG, "unknown metric");
    return assign_impl(ctx, X, N, lsh->proj.d, C, K, metric, src_rows_host, assign, dist, lsh, tuples, phi, bucket);
}

static int range_impl(lshkm_ctx ctx, Pts X, int64_t N, int d, const double* C, int K, int metric,
                      const int64_t* comb_ptr, const int32_t* comb_idx, const int32_t* key_host,
                      const int32_t* src_rows_host, int32_t* assign, double* dist, int* passes_host) {
    LSHKM_CHECK(ctx && (X.p || N == 0) && C && comb_ptr && (assign || N == 0) && (dist || N == 0) && N >= 0 &&
                    N < (1ll << 31) && d > 0 && K > 0,
                LSHKM_ERR_ARG, "bad arguments");
    LSHKM_CHECK(metric == LSHKM_METRIC_EUCLIDEAN || metric == LSHKM_METRIC_COSINE, LSHKM_ERR_ARG, "unknown metric");
    LSHKM_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    lshkm::Buf* w = ctx->ws_range;
    int rc;
    int64_t M = 0;
    LSHKM_HIP(hipMemcpyAsync(&M, comb_ptr + K, 8, hipMemcpyDeviceToHost, s));
    LSHKM_HIP(hipStreamSynchronize(s));
    LSHKM_CHECK(M >= 0 && (M == 0 || comb_idx), LSHKM_ERR_ARG, "bad combined-bucket CSR");
    const size_t scratch = sort_scratch_bytes(std::max<int64_t>(M, 1), std::max<int64_t>(N, 1));
    if ((rc = w[0].reserve(64)) || (rc = w[1].reserve((size_t)std::max<int64_t>(M, 1) * 4 * 4)) ||
        (rc = w[2].reserve(scratch)) || (rc = w[3].reserve((size_t)(N + 1) * 8)) ||
        (rc = w[4].reserve((size_t)std::max<int64_t>(M, 1) * 9)) || (rc = w[5].reserve((size_t)K * 4)))
        return rc;
    double* r0 = (double*)w[0].p;                          // [0] r0, [1] pass count, [2] unassigned count
    unsigned long long* cnt = (unsigned long long*)w[0].p + 1;
    int32_t* rows = (int32_t*)w[1].p;
    int32_t* cents = rows + std::max<int64_t>(M, 1);
    int32_t* rows_s = cents + std::max<int64_t>(M, 1);
    int32_t* cents_s = rows_s + std::max<int64_t>(M, 1);
    int64_t* vptr = (int64_t*)w[3].p;
    double* cache = (double*)w[4].p;
    int8_t* cached = (int8_t*)(cache + std::max<int64_t>(M, 1));
    const int32_t* key = nullptr;
    if (key_host) {
        LSHKM_HIP(hipMemcpyAsync(w[5].p, key_host, (size_t)K * 4, hipMemcpyHostToDevice, s));
        key = (const int32_t*)w[5].p;
    }
    if ((rc = launch_range_radius(s, C, K, d, metric, r0, (unsigned long long*)w[0].p + 4))) return rc;
    if ((rc = launch_range_init(s, N, assign, dist))) return rc;
    int passes = 0;
    if (M > 0 && N > 0) {
        if ((rc = launch_range_pairs(s, comb_ptr, comb_idx, K, rows, cents))) return rc;
        if ((rc = stable_sort_by_key(s, rows, 1, cents, M, N, rows_s, cents_s, w[2].p))) return rc;
        if ((rc = launch_csr_bounds(s, rows_s, M, N, vptr))) return rc;
        LSHKM_HIP(hipMemsetAsync(cached, 0, (size_t)M, s));
        // the do-while of assignment.hpp:160-216, one launch per pass
        for (;;) {
            unsigned long long assigned = 0;
            LSHKM_HIP(hipMemsetAsync(cnt, 0, 8, s));
            if ((rc = launch_range_pass(s, X, d, C, K, metric, key, vptr, cents_s, cache, cached, N, r0, passes,
                                        assign, dist, cnt)))
                return rc;
            passes++;
            LSHKM_HIP(hipMemcpyAsync(&assigned, cnt, 8, hipMemcpyDeviceToHost, s));
            LSHKM_HIP(hipStreamSynchronize(s));
            if (!assigned) break;
        }
    } else {
        passes = 1;     // one pass over empty buckets assigns nothing
    }
    // lloyds_for_remaining (assignment.hpp:83-104): the Lloyd path on the rows left unassigned
    if (N > 0) {
        if ((rc = w[6].reserve((size_t)N * 4))) return rc;
        int32_t* list = (int32_t*)w[6].p;
        unsigned long long* ucnt = cnt + 1;
        unsigned long long U = 0;
        LSHKM_HIP(hipMemsetAsync(ucnt, 0, 8, s));
        if ((rc = launch_range_unassigned(s, assign, N, list, ucnt))) return rc;
        LSHKM_HIP(hipMemcpyAsync(&U, ucnt, 8, hipMemcpyDeviceToHost, s));
        LSHKM_HIP(hipStreamSynchronize(s));
        if (U > 0) {
            if ((rc = w[7].reserve((size_t)U * d * X.esize())) || (rc = w[8].reserve((size_t)U * 12))) return rc;
            double* dr = (double*)w[8].p;
            int32_t* ar = (int32_t*)(dr + U);
            if ((rc = launch_range_gather(s, X, d, list, (int64_t)U, w[7].p))) return rc;
            const Pts Xr = X.f64 ? Pts(w[7].as<double>()) : Pts(w[7].as<float>());
            // the range pass's distances are the exact chain; the leftover rows
            // get the same (a range assignment is exact-order in either mode)
            rc = assign_impl(ctx, Xr, (int64_t)U, d, C, K, metric, nullptr, ar, dr, nullptr, nullptr, nullptr, nullptr,
                             true);
            if (rc) return rc;
            if ((rc = launch_range_scatter(s, list, (int64_t)U, ar, dr, assign, dist))) return rc;
        }
    }
    // the centroid override (assignment.hpp:125-127, :143-145)
    if (src_rows_host) {
        if ((rc = ctx->ws_src.reserve((size_t)K * 4))) return rc;
        ctx->src_cache_dev = nullptr;            // ws_src overwritten outside the cache
        LSHKM_HIP(hipMemcpyAsync(ctx->ws_src.p, src_rows_host, (size_t)K * 4, hipMemcpyHostToDevice, s));
        if ((rc = launch_assign_override(s, (const int32_t*)ctx->ws_src.p, K, N, assign, dist))) return rc;
        LSHKM_HIP(hipStreamSynchronize(s));     // the host arrays may be freed on return
    }
    if (key_host) LSHKM_HIP(hipStreamSynchronize(s));
    if (passes_host) *passes_host = passes;
    return 0;
}

extern "C" {

int lshkm_lloyd_assign(lshkm_ctx ctx, const float* X, int64_t N, int d, const double* C, int K, int metric,
                       const int32_t* src_rows_host, int32_t* assign, double* dist) {
    return lloyd_impl(ctx, X, N, d, C, K, metric, src_rows_host, assign, dist);
}

int lshkm_lloyd_assign_f64(lshkm_ctx ctx, const double* X, int64_t N, int d, const double* C, int K, int metric,
                           const int32_t* src_rows_host, int32_t* assign, double* dist) {
    return lloyd_impl(ctx, X, N, d, C, K, metric, src_rows_host, assign, dist);
}

int lshkm_hash_assign(lshkm_lsh lsh, const float* X, int64_t N, const double* C, int K, const int32_t* src_rows_host,
                      int32_t* tuples, int32_t* phi, int32_t* bucket, int32_t* assign, double* dist) {
    return hash_assign_impl(lsh, X, N, C, K, src_rows_host, tuples, phi, bucket, assign, dist);
}

int lshkm_hash_assign_f64(lshkm_lsh lsh, const double* X, int64_t N, const double* C, int K,
                          const int32_t* src_rows_host, int32_t* tuples, int32_t* phi, int32_t* bucket,
                          int32_t* assign, double* dist) {
    return hash_assign_impl(lsh, X, N, C, K, src_rows_host, tuples, phi, bucket, assign, dist);
}

int lshkm_hash_assign_metric(lshkm_lsh lsh, const float* X, int64_t N, const double* C, int K, int metric,
                             const int32_t* src_rows_host, int32_t* tuples, int32_t* phi, int32_t* bucket,
                             int32_t* assign, double* dist) {
    return hash_assign_impl(lsh, X, N, C, K, src_rows_host, tuples, phi, bucket, assign, dist, metric);
}

int lshkm_hash_assign_metric_f64(lshkm_lsh lsh, const double* X, int64_t N, const double* C, int K, int metric,
                                 const int32_t* src_rows_host, int32_t* tuples, int32_t* phi, int32_t* bucket,
                                 int32_t* assign, double* dist) {
    return hash_assign_impl(lsh, X, N, C, K, src_rows_host, tuples, phi, bucket, assign, dist, metric);
}

int lshkm_range_assign(lshkm_ctx ctx, const float* X, int64_t N, int d, const double* C, int K, int metric,
                       const int64_t* comb_ptr, const int32_t* comb_idx, const int32_t* key_host,
                       const int32_t* src_rows_host, int32_t* assign, double* dist, int* passes_host) {
    return range_impl(ctx, X, N, d, C, K, metric, comb_ptr, comb_idx, key_host, src_rows_host, assign, dist,
                      passes_host);
}

int lshkm_range_assign_f64(lshkm_ctx ctx, const double* X, int64_t N, int d, const double* C, int K, int metric,
                           const int64_t* comb_ptr, const int32_t* comb_idx, const int32_t* key_host,
                           const int32_t* src_rows_host, int32_t* assign, double* dist, int* passes_host) {
    return range_impl(ctx, X, N, d, C, K, metric, comb_ptr, comb_idx, key_host, src_rows_host, assign, dist,
                      passes_host);
}

int lshkm_synth(lshkm_ctx ctx, uint64_t seed, int64_t row0, int64_t rows, int d, float* X) {
    LSHKM_CHECK(ctx && (X || rows == 0) && rows >= 0 && d > 0, LSHKM_ERR_ARG, "bad arguments");
    LSHKM_HIP(hipSetDevice(ctx->device));
    int rc = launch_synth(ctx->stream, seed, row0, rows, d, X);
    if (rc) { LSHKM_LAUNCH_CHECK(); }
    return rc;
}

int lshkm_synth_normal(lshkm_ctx ctx, uint64_t seed, int64_t row0, int64_t rows, int d, float* X) {
    LSHKM_CHECK(ctx && (X || rows == 0) && rows >= 0 && d > 0, LSHKM_ERR_ARG, "bad arguments");
    LSHKM_HIP(hipSetDevice(ctx->device));
    int rc = launch_synth(ctx->stream, seed, row0, rows, d, X, 1);
    if (rc) { LSHKM_LAUNCH_CHECK(); }
    return rc;
}

}  // extern "C"
