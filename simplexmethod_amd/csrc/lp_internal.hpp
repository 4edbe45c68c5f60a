// lp_internal.hpp — shared host-side plumbing for the HIP hot path (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/simplexmethod_amd.h"

struct lp_context {
    int device = -1;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    int num_cus = 0;
    size_t total_mem = 0;   // device memory (queried on first use)
    std::string last_error;
    // Large device buffers released by freed problems, kept for the next one (hipMalloc / hipFree of
    // the enumeration's multi-GB level buffers cost milliseconds: more than a small solve).
    std::vector<std::pair<void*, size_t>> pool;
    // shape-independent subset tables of the enumeration's leaf kernels, built once per context
    unsigned* dcomb6 = nullptr;
    unsigned* dcomb5 = nullptr;
    unsigned* dcomb4 = nullptr;
    // three more streams + events (created on first use): the enumeration's independent leaf kernels run
    // side by side so that one kernel's tail is filled by the next one's head
    hipStream_t aux_stream[3] = {nullptr, nullptr, nullptr};
    hipEvent_t aux_event[4] = {nullptr, nullptr, nullptr, nullptr};
    // freed enumeration problems with every allocation intact (their ~20 device / pinned allocations
    // and events cost more than a C(28,14) solve); lp_enum_upload refills one instead of allocating
    std::vector<void*> enum_shells;
    // pinned state blocks and event sets of freed simplex problems (hipHostMalloc / hipEventCreate
    // cost more than a small solve)
    struct HostBundle {
        void* pinned = nullptr;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    };
    std::vector<HostBundle> bundles;
};

// Best-fit buffer of at least `bytes` from the context's pool (not more than twice as large), else
// hipMalloc.  *got receives the actual size.
inline hipError_t lp_pool_alloc(lp_context* ctx, void** out, size_t bytes, size_t* got) {
    int best = -1;
    for (int k = 0; k < (int)ctx->pool.size(); ++k) {
        const size_t have = ctx->pool[(size_t)k].second;
        if (have >= bytes && have <= 2 * bytes + (1u << 20) &&
            (best < 0 || have < ctx->pool[(size_t)best].second))
            best = k;
    }
    if (best >= 0) {
        *out = ctx->pool[(size_t)best].first;
        *got = ctx->pool[(size_t)best].second;
        ctx->pool.erase(ctx->pool.begin() + best);
        return hipSuccess;
    }
    *got = bytes;
    return hipMalloc(out, bytes);
}
inline void lp_pool_release(lp_context* ctx, void* p, size_t bytes) {
    if (!p) return;
    constexpr size_t kMaxPooled = 8;
    if (bytes < (1u << 20) || ctx->pool.size() >= kMaxPooled) {
        (void)hipFree(p);
        return;
    }
    ctx->pool.emplace_back(p, bytes);
}

// HIP call check: records the message in the context and returns -(hipError_t).
#define LP_HIP(ctx, expr)                                                                  \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            char _buf[512];                                                                \
            snprintf(_buf, sizeof(_buf), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,     \
                     hipGetErrorString(_e));                                               \
            (ctx)->last_error = _buf;                                                      \
            return -(int)_e;                                                               \
        }                                                                                  \
    } while (0)

#define LP_FAIL(ctx, code, msg)      \
    do {                             \
        (ctx)->last_error = (msg);   \
        return (code);               \
    } while (0)

// Owns one device allocation for the length of a call: freed on every return path.
struct lp_device_buffer {
    char* ptr = nullptr;
    lp_device_buffer() = default;
    lp_device_buffer(const lp_device_buffer&) = delete;
    lp_device_buffer& operator=(const lp_device_buffer&) = delete;
    ~lp_device_buffer() { (void)hipFree(ptr); }
};

// Hands out 16-byte-aligned pieces of one device allocation in the order they are asked for.  A carve list runs
// twice through lp_carve_malloc: first on a carver without a base, which only measures, then over the allocation,
// so the allocation's size always comes from the list that hands out the pointers.
struct lp_carver {
    char* base = nullptr;
    size_t used = 0;
    template <typename T>
    T* take(size_t bytes) {
        T* r = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += (bytes + 15) & ~(size_t)15;
        return r;
    }
};

// hipMalloc of exactly what `list(lp_carver&)` takes, then `list` again over the allocation.
template <typename List>
inline hipError_t lp_carve_malloc(char** arena, List&& list) {
    lp_carver measure;
    list(measure);
    const hipError_t e = hipMalloc(arena, measure.used);
    if (e != hipSuccess) return e;
    lp_carver cut{*arena};
    list(cut);
    return hipSuccess;
}

// One device-to-host copy of lp_download.
struct lp_d2h {
    void* dst;
    const void* src;
    size_t bytes;
};

// Queues the copies on the context's stream (those of 0 bytes are skipped), then one sync.  A failure is
// "<label>: <HIP error>" in last_error and -(hipError_t) returned.
inline int lp_download(lp_context* ctx, const char* label, std::initializer_list<lp_d2h> copies) {
    hipError_t e = hipSuccess;
    for (const lp_d2h& q : copies)
        if (e == hipSuccess && q.bytes) e = hipMemcpyAsync(q.dst, q.src, q.bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string(label) + ": " + hipGetErrorString(e));
    return LP_OPTIMAL;
}

template <typename T>
static inline T lp_ceil_div(T a, T b) {
    return (a + b - 1) / b;
}

// The pivot rules the _ex entries and the two setters accept.
static inline bool lp_pivot_rule_known(int rule) {
    return rule == LP_PIVOT_DANTZIG || rule == LP_PIVOT_BLAND || rule == LP_PIVOT_DEVEX;
}

// The dual pricing rules the _dual_ex entries accept.
static inline bool lp_dual_rule_known(int rule) { return rule == LP_DUAL_DANTZIG || rule == LP_DUAL_DEVEX; }

// The dual ratio tests the _ratio_ex entries accept.
static inline bool lp_dual_ratio_known(int ratio) { return ratio == LP_DUAL_RATIO_TEXTBOOK || ratio == LP_DUAL_RATIO_LONG_STEP; }

// Host-side combinatorics shared by the enumeration paths (exact u64; 0 = overflow).
uint64_t lp_host_binom(int n, int k);
// rank, among the t-subsets of {0 .. n-m+t-1}, of the first t elements of the rank-th m-subset of
// {0 .. n-1} (enum_driver.hip)
uint64_t lp_host_prefix_rank(int n, int m, uint64_t rank, int t);
