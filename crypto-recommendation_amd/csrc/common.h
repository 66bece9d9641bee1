// common.h — shared internals of liblshkm (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#ifdef LSHKM_TEST_SWITCHES
#include <cstdlib>
#include <cstring>
#endif

namespace lshkm {

// Path switches for the tests' A/B comparisons (one kernel path forced against
// another, bit for bit). Compiled only into the test build liblshkm_test.so
// (-DLSHKM_TEST_SWITCHES, `make test`); the product library liblshkm.so reads
// no environment and always takes the default paths.
inline bool test_switch(const char* name, const char* value) {
#ifdef LSHKM_TEST_SWITCHES
    const char* e = std::getenv(name);
    return e && !std::strcmp(e, value);
#else
    (void)name;
    (void)value;
    return false;
#endif
}

// Thread-local last error, surfaced through lshkm_last_error().
void set_error(const std::string& msg);

#define LSHKM_HIP(expr)                                                              \
    do {                                                                             \
        hipError_t _e = (expr);                                                      \
        if (_e != hipSuccess) {                                                      \
            ::lshkm::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));   \
            return LSHKM_ERR_HIP;                                                    \
        }                                                                            \
    } while (0)

#define LSHKM_CHECK(cond, code, msg)                                                 \
    do {                                                                             \
        if (!(cond)) { ::lshkm::set_error(msg); return code; }                       \
    } while (0)

#define LSHKM_LAUNCH_CHECK() LSHKM_HIP(hipGetLastError())

// Status of the launches just issued by a launcher: 0, or -2 with the HIP
// error recorded for lshkm_last_error().
inline int kstatus(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return -2;
}

// Wave-scope LDS handoff: makes one lane's LDS writes visible to the other
// lanes of its wave (a fence the compiler cannot move loads across).
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Append this lane's entry (where want) to a list segment with fill count
// *count (LDS or global): one atomic per wave by its first wanting lane, the
// entries in lane order. Every lane that can want calls it together. (The fused
// pass's kernels keep the idiom written out: profiles/README.md.)
template <typename E, typename C>
__device__ __forceinline__ void seg_append(bool want, E entry, C* count, E* seg, int lane) {
    const unsigned long long m = __ballot(want);
    if (!m) return;
    const int leader = __builtin_ctzll(m);
    C base = 0;
    if (lane == leader) base = atomicAdd(count, (C)__popcll(m));
    base = __shfl(base, leader);
    if (want) seg[base + __popcll(m & ((1ull << lane) - 1ull))] = entry;
}

// Grid size for a grid-stride kernel: at least one block, at most cap.
inline unsigned gsz(int64_t work, int64_t per_block, int64_t cap) {
    int64_t b = (work + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// Device counters kept per context (see lshkm_get_stat).
enum Stat {
    STAT_HASH_EXACT = 0,     // hash values resolved by the soft-x87 exact path
    STAT_ASSIGN_AMBIG = 1,   // points whose argmin the MFMA bound could not certify
    STAT_KPP_CHUNKS = 2,     // k-means++ prefix-walk chunks (KPP_CHUNK rows each) ...
    STAT_KPP_SEQ = 3,        // ... of which summed element by element (binade crossings, ties)
    STAT_COS_FIX = 4,        // cosine Lloyd winners whose distance took the soft-x87 chain
    STAT_REFINED = 5,        // rows the hi-only fused pass left to the 3-product refinement
    STAT_HASH_FIX = 6,       // rows the fused pass listed for the hash fix-up (an uncertified floor / sign)
    STAT_REC_SOFT = 7,       // clustering-recommender similarities decided by the x87 chain (IpAcc declined)
    STAT_POW_FIX = 8,        // euclidean winner distances redone with glibc's pow(x, 2) (an inexact square)
    STAT_KM_SEQ = 9,         // k-means (cluster, dim) sums whose never-rounds test failed (sequential / segment chain)
    STAT_PAM_SCREENED = 10,  // PAM update: clusters whose argmin went through the MFMA screen
    STAT_PAM_EXACT = 11,     // ... and the members the screen left to the exact chain
    STAT_LSHPC_SETTLED = 12, // lshkm_lsh_p_closest / lshkm_cube_p_closest: users the MFMA screen settled
    STAT_LSHPC_LISTS = 13,   // ... users sent to the lists path (poison, overflow, tie / NaN; or the whole call)
    STAT_LSHPC_KEPT = 14,    // ... candidates the screen kept for the exact pass
    STAT_LSHPC_SEEN = 15,    // ... candidates it saw
    STAT_PAIR_ROWS = 16,     // rows of STAT_ASSIGN_AMBIG the refinement named both candidates of and decided itself
    STAT_NEAREST_SETTLED = 17, // lshkm_min_vector_dist: queries the MFMA screen settled
    STAT_NEAREST_SCAN = 18,  // ... queries sent to the exact scan over all rows (poison, overflow; or the whole call)
    STAT_NEAREST_EXACT = 19, // ... exact distances the settle computed (the lists form's too)
    STAT_KNN_SETTLED = 20,   // lshkm_knn: queries the MFMA screen settled
    STAT_KNN_SCAN = 21,      // ... queries sent to the exact scan over all rows (poison, no threshold, overflow; or the whole call)
    STAT_KNN_EXACT = 22,     // ... exact distances the settle computed (the lists form's too)
    STAT_COUNT = 23
};

constexpr int WAVE = 64;

// CUs of the current device (cached, thread-safe); 0, or -2 with the HIP error recorded.
int device_cu_count(int* ncu);

}  // namespace lshkm
