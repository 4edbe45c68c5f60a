// capi.hip — the extern "C" boundary (include/simplexmethod_amd.h): the context, the status strings and the
// division self-tests.  The single-LP simplex is simplex_driver.hip, the enumeration enum_driver.hip, the batch
// handle (plain, two-phase and re-solve batches) and the bounded-variable simplex batched_driver.hip, and every
// analysis that starts from an LP and a basis (duals, ranging, certificates, parametric RHS and cost,
// branch-and-bound) basis_driver.hip.
#include <cstring>

#include "enum_problem.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

uint64_t lp_host_binom(int n, int k) {
    if (k < 0 || k > n) return 0;
    if (k > n - k) k = n - k;
    unsigned __int128 r = 1;
    for (int i = 1; i <= k; ++i) {
        r = r * (unsigned)(n - k + i) / (unsigned)i;
        if (r > (unsigned __int128)UINT64_MAX) return 0;
    }
    return (uint64_t)r;
}

extern "C" {

int lp_abi_version(void) { return LP_ABI_VERSION; }

int lp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* lp_status_string(int status) {
    switch (status) {
        case LP_OPTIMAL: return "optimal";
        case LP_UNBOUNDED: return "objective unbounded";
        case LP_ITER_LIMIT: return "iteration limit reached";
        case LP_SINGULAR: return "singular basis matrix";
        case LP_INFEASIBLE: return "no feasible basis";
        case LP_BAD_ARG: return "bad argument";
        default: return status < 0 ? "HIP runtime error" : "unknown status";
    }
}

static thread_local std::string g_create_error;

int lp_context_create(int device, void* stream, lp_context** ctx_out) {
    if (!ctx_out) return LP_BAD_ARG;
    *ctx_out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_error = "no HIP device visible (this library has no CPU fallback)";
        return e != hipSuccess ? -(int)e : -(int)hipErrorNoDevice;
    }
    if (device < 0 || device >= count) return LP_BAD_ARG;
    e = hipSetDevice(device);
    if (e != hipSuccess) return -(int)e;
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return -(int)e;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName +
                         ", kernels are built for gfx950 only";
        return -(int)hipErrorNoBinaryForGpu;
    }
    lp_context* ctx = new lp_context();
    ctx->device = device;
    ctx->num_cus = prop.multiProcessorCount;
    if (stream) {
        ctx->stream = (hipStream_t)stream;
    } else {
        e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete ctx;
            return -(int)e;
        }
        ctx->owns_stream = true;
    }
    *ctx_out = ctx;
    return LP_OPTIMAL;
}

void lp_context_destroy(lp_context* ctx) {
    if (!ctx) return;
    lp_enum_release_shells(ctx);
    for (auto& b : ctx->pool) (void)hipFree(b.first);
    for (auto& hb : ctx->bundles) {
        (void)hipHostFree(hb.pinned);
        for (hipEvent_t e : hb.ev)
            if (e) (void)hipEventDestroy(e);
    }
    (void)hipFree(ctx->dcomb6);
    (void)hipFree(ctx->dcomb5);
    (void)hipFree(ctx->dcomb4);
    for (hipStream_t a : ctx->aux_stream)
        if (a) (void)hipStreamDestroy(a);
    for (hipEvent_t e : ctx->aux_event)
        if (e) (void)hipEventDestroy(e);
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* lp_last_error(const lp_context* ctx) {
    return ctx ? ctx->last_error.c_str() : g_create_error.c_str();
}

int lp_context_sync(lp_context* ctx) {
    if (!ctx) return LP_BAD_ARG;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    LP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LP_OPTIMAL;
}

// ===========================================================================
// diagnostics of the kernels' fast divisions (the enumeration's C ABI: enum_driver.hip)
// ===========================================================================

int lp_debug_reciprocal(lp_context* ctx, const double* x, int n, double* fast_out, double* plain_out) {
    if (!ctx || !x || !fast_out || !plain_out || n <= 0) return LP_BAD_ARG;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    return lp_enum_debug_reciprocal(ctx, x, n, fast_out, plain_out);
}

int lp_debug_division(lp_context* ctx, const double* num, const double* den, int n, double* fast_out, double* plain_out) {
    if (!ctx || !num || !den || !fast_out || !plain_out || n <= 0) return LP_BAD_ARG;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    return lp_simplex_debug_division(ctx, num, den, n, fast_out, plain_out);
}

}  // extern "C"
