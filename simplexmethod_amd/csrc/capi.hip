// capi.hip — the extern "C" boundary (include/simplexmethod_amd.h): the context, the status strings, the
// division self-tests, the batched simplex handle (plain, two-phase and re-solve batches) and the bounded-variable
// simplex.  The single-LP simplex is simplex_driver.hip, the enumeration enum_driver.hip, and every analysis that
// starts from an LP and a basis (duals, ranging, certificates, parametric RHS and cost, branch-and-bound)
// basis_driver.hip.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "batched_problem.hpp"
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

// ===========================================================================
// batched simplex — one LP per workgroup (batched_simplex.hip).  LPs whose initial
// basis is not the slack identity, or whose condensed tableau does not fit one CU's
// LDS, go through the single-LP path one after another instead.
// A batch uploaded by lp_batched_two_phase_upload has no starting basis and runs the
// two-phase flow, one LP per workgroup (batched_two_phase.hip); shapes that do not fit
// go through lp_simplex_two_phase one LP after another.  A batch uploaded by lp_batched_resolve_upload is
// re-solved from its given bases (batched_resolve.hip).
// ===========================================================================

void lp_batched_free(lp_batched_problem* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    for (auto* q : p->lps) lp_simplex_free(q);
    (void)hipFree(p->dA); (void)hipFree(p->db); (void)hipFree(p->dc); (void)hipFree(p->dx);
    (void)hipFree(p->dbasis_in); (void)hipFree(p->dbasis_out); (void)hipFree(p->diters);
    (void)hipFree(p->dstatus); (void)hipFree(p->dev.stamps);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    delete p;
}

int lp_batched_set_pivot_rule(lp_batched_problem* p, int pivot_rule) {
    if (!p) return LP_BAD_ARG;
    if (pivot_rule != LP_PIVOT_DANTZIG && pivot_rule != LP_PIVOT_BLAND)
        LP_FAIL(p->ctx, LP_BAD_ARG, "unknown pivot rule");
    p->pivot_rule = pivot_rule;
    return LP_OPTIMAL;
}

int lp_batched_shard_bounds(int batch, int shard, int shards, int* lo, int* hi) {
    if (batch < 0 || shards < 1 || shard < 0 || shard >= shards || !lo || !hi) return LP_BAD_ARG;
    *lo = (int)((long long)batch * shard / shards);
    *hi = (int)((long long)batch * (shard + 1) / shards);
    return LP_OPTIMAL;
}

int lp_batched_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                      const double* c, const int* basis_in, int maximize, int n_orig,
                      lp_batched_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    for (int k = 0; k < batch; ++k) {
        int rc = check_canonical(ctx, A ? A + (size_t)k * m * n : nullptr, m, n,
                                 b ? b + (size_t)k * m : nullptr, c ? c + (size_t)k * n : nullptr,
                                 basis_in ? basis_in + (size_t)k * m : nullptr, n_orig);
        if (rc) return rc;
    }
    LP_HIP(ctx, hipSetDevice(ctx->device));
    lp_batched_problem* p = new lp_batched_problem();
    p->ctx = ctx;
    p->batch = batch;
    p->m = m;
    p->n = n;
    p->n_orig = n_orig;
    p->status.assign((size_t)batch, -100);
    p->iters.assign((size_t)batch, 0);
    p->h_c.assign(c, c + (size_t)batch * n);
    // resident path needs: slack identity basis with zero basic costs in every LP, n > m,
    // and the condensed tableau within one CU's LDS
    bool identity = n > m;
    for (int k = 0; k < batch && identity; ++k) {
        bool zero_costs = true;
        lp_slack_identity(A + (size_t)k * m * n, m, c + (size_t)k * n, basis_in + (size_t)k * m, &identity, &zero_costs);
        identity = identity && zero_costs;
    }
    int pitch = 0;
    const size_t lds = lp_batched_lds_bytes(m, n, &pitch);
    p->resident = identity && lds <= 160 * 1024;
    p->maximize = maximize ? 1 : 0;   // (the sense lp_batched_ranging reads)
    if (!p->resident) {   // per-LP fallback; the inputs are kept for lp_batched_duals
        p->h_A.assign(A, A + (size_t)batch * m * n);
        p->h_b.assign(b, b + (size_t)batch * m);
        for (int k = 0; k < batch; ++k) {
            lp_simplex_problem* q = nullptr;
            int rc = lp_simplex_upload(ctx, A + (size_t)k * m * n, m, n, b + (size_t)k * m,
                                       c + (size_t)k * n, basis_in + (size_t)k * m, maximize,
                                       n_orig, &q);
            if (rc) {
                lp_batched_free(p);
                return rc;
            }
            p->lps.push_back(q);
        }
        *problem_out = p;
        return LP_OPTIMAL;
    }
#define LP_TRY(expr)                        \
    do {                                    \
        hipError_t _e = (expr);             \
        if (_e != hipSuccess) {             \
            ctx->last_error = #expr;        \
            lp_batched_free(p);             \
            return -(int)_e;                \
        }                                   \
    } while (0)
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch;
    LP_TRY(hipMalloc(&p->dA, sizeof(double) * B * m * n));
    LP_TRY(hipMalloc(&p->db, sizeof(double) * B * m));
    LP_TRY(hipMalloc(&p->dc, sizeof(double) * B * n));
    LP_TRY(hipMalloc(&p->dx, sizeof(double) * B * n));
    LP_TRY(hipMalloc(&p->dbasis_in, sizeof(int) * B * m));
    LP_TRY(hipMalloc(&p->dbasis_out, sizeof(int) * B * m));
    LP_TRY(hipMalloc(&p->diters, sizeof(int) * B));
    LP_TRY(hipMalloc(&p->dstatus, sizeof(int) * B));
    LP_TRY(hipEventCreate(&p->ev0));
    LP_TRY(hipEventCreate(&p->ev1));
    LP_TRY(hipMemcpyAsync(p->dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->dbasis_in, basis_in, sizeof(int) * B * m, hipMemcpyHostToDevice, s));
    LP_TRY(hipStreamSynchronize(s));
#undef LP_TRY
    BatchedDev& d = p->dev;
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.pitch = pitch;
    d.maximize = maximize ? 1 : 0;
    d.A = p->dA;
    d.b = p->db;
    d.c = p->dc;
    d.basis_in = p->dbasis_in;
    d.x = p->dx;
    d.basis_out = p->dbasis_out;
    d.iters = p->diters;
    d.status = p->dstatus;
    *problem_out = p;
    return LP_OPTIMAL;
}

int lp_batched_two_phase_upload(lp_context* ctx, int batch, const double* A, int m, int n,
                                const double* b, const double* c, int maximize, int n_orig,
                                lp_batched_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    // the checks of lp_simplex_two_phase
    if (!A || !b || !c) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_two_phase_upload: null argument");
    if (m <= 0 || n < m || n_orig <= 0 || n_orig > n)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_two_phase_upload: bad dimensions");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    lp_batched_problem* p = new lp_batched_problem();
    p->ctx = ctx;
    p->two_phase = true;
    p->batch = batch;
    p->m = m;
    p->n = n;
    p->n_orig = n_orig;
    p->maximize = maximize ? 1 : 0;
    const size_t B = (size_t)batch;
    p->status.assign(B, -100);
    p->phase_iters.assign(B * 3, 0);
    p->h_c.assign(c, c + B * n);
    p->resident = lp_batched_two_phase_fits(m, n);
    if (!p->resident) {   // per-LP fallback: keep the inputs for lp_simplex_two_phase
        p->h_A.assign(A, A + B * m * n);
        p->h_b.assign(b, b + B * m);
        p->h_x.assign(B * n_orig, 0.0);
        p->h_obj.assign(B, 0.0);
        p->h_basis.assign(B * m, -1);
        *problem_out = p;
        return LP_OPTIMAL;
    }
#define LP_TRY(expr)                        \
    do {                                    \
        hipError_t _e = (expr);             \
        if (_e != hipSuccess) {             \
            ctx->last_error = #expr;        \
            lp_batched_free(p);             \
            return -(int)_e;                \
        }                                   \
    } while (0)
    hipStream_t s = ctx->stream;
    LP_TRY(hipMalloc(&p->dA, sizeof(double) * B * m * n));
    LP_TRY(hipMalloc(&p->db, sizeof(double) * B * m));
    LP_TRY(hipMalloc(&p->dc, sizeof(double) * B * n));
    LP_TRY(hipMalloc(&p->dx, sizeof(double) * B * n));
    LP_TRY(hipMalloc(&p->dbasis_out, sizeof(int) * B * m));
    LP_TRY(hipMalloc(&p->diters, sizeof(int) * B * 3));
    LP_TRY(hipMalloc(&p->dstatus, sizeof(int) * B));
    LP_TRY(hipEventCreate(&p->ev0));
    LP_TRY(hipEventCreate(&p->ev1));
    LP_TRY(hipMemcpyAsync(p->dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s));
    LP_TRY(hipStreamSynchronize(s));
#undef LP_TRY
    BatchedTwoPhaseDev& d = p->tdev;
    d.batch = batch;
    d.m = m;
    d.n = n;
    (void)lp_batched_two_phase_lds_bytes(m, n, &d.pitch);
    d.maximize = p->maximize;
    d.A = p->dA;
    d.b = p->db;
    d.c = p->dc;
    d.x = p->dx;
    d.basis_out = p->dbasis_out;
    d.iters = p->diters;
    d.status = p->dstatus;
    *problem_out = p;
    return LP_OPTIMAL;
}

static int batched_two_phase_run(lp_batched_problem* p, double eps, int max_iter, float* ms_out) {
    lp_context* ctx = p->ctx;
    if (p->resident) {
        p->tdev.eps = eps;
        p->tdev.max_iter = max_iter;
        LP_HIP(ctx, hipEventRecord(p->ev0, ctx->stream));
        int rc = lp_batched_two_phase_launch(ctx, p->tdev, p->pivot_rule);
        if (rc) return rc;
        LP_HIP(ctx, hipGetLastError());
        LP_HIP(ctx, hipEventRecord(p->ev1, ctx->stream));
        LP_HIP(ctx, hipEventSynchronize(p->ev1));
        float ms = 0.f;
        LP_HIP(ctx, hipEventElapsedTime(&ms, p->ev0, p->ev1));
        if (ms_out) *ms_out = ms;
        return LP_OPTIMAL;
    }
    // per-LP fallback: lp_simplex_two_phase one LP after another (host clock)
    const auto t0 = std::chrono::steady_clock::now();
    const int m = p->m, n = p->n;
    for (int k = 0; k < p->batch; ++k) {
        int rc = lp_simplex_two_phase_ex(ctx, p->h_A.data() + (size_t)k * m * n, m, n, p->h_b.data() + (size_t)k * m,
                                         p->h_c.data() + (size_t)k * n, p->maximize, p->n_orig, eps, max_iter,
                                         p->h_x.data() + (size_t)k * p->n_orig, p->h_basis.data() + (size_t)k * m,
                                         p->h_obj.data() + k, p->phase_iters.data() + (size_t)k * 3, p->pivot_rule);
        if (rc < 0 || rc > LP_INFEASIBLE) return rc;
        p->status[(size_t)k] = rc;
    }
    if (ms_out) *ms_out = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return LP_OPTIMAL;
}

static int batched_two_phase_download(lp_batched_problem* p, double* x_out, int* basis_out, double* obj_out,
                                      int* iters_out, int* status_out) {
    lp_context* ctx = p->ctx;
    const size_t B = (size_t)p->batch;
    const int m = p->m, n = p->n, no = p->n_orig;
    std::vector<double> x;
    if (p->resident) {
        x.resize(B * n);
        hipStream_t s = ctx->stream;
        LP_HIP(ctx, hipMemcpyAsync(x.data(), p->dx, sizeof(double) * B * n, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipMemcpyAsync(p->status.data(), p->dstatus, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipMemcpyAsync(p->phase_iters.data(), p->diters, sizeof(int) * B * 3, hipMemcpyDeviceToHost, s));
        if (basis_out) LP_HIP(ctx, hipMemcpyAsync(basis_out, p->dbasis_out, sizeof(int) * B * m, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipStreamSynchronize(s));
    } else if (basis_out) {
        std::memcpy(basis_out, p->h_basis.data(), sizeof(int) * B * m);
    }
    for (size_t k = 0; k < B; ++k) {
        const bool ok = p->status[k] == LP_OPTIMAL;
        if (p->resident && ok) {
            const double* xk = x.data() + k * n;
            if (x_out)  // x.head(n_orig)
                for (int j = 0; j < no; ++j) x_out[k * no + j] = xk[j];
            if (obj_out) {  // Canonical::Evaluate, Canonical.cpp:86
                double z = 0.0;
                const double* ck = p->h_c.data() + k * n;
                for (int j = 0; j < n; ++j) z += ck[j] * xk[j];
                obj_out[k] = z;
            }
        } else if (ok) {
            if (x_out) std::memcpy(x_out + k * no, p->h_x.data() + k * no, sizeof(double) * no);
            if (obj_out) obj_out[k] = p->h_obj[k];
        }
        const int* it = p->phase_iters.data() + k * 3;
        if (iters_out) iters_out[k] = it[0] + it[1] + it[2];
        if (status_out) status_out[k] = p->status[k];
    }
    return LP_OPTIMAL;
}

// ===========================================================================
// re-solve batch: every LP from its given basis, primal or dual simplex (batched_resolve.hip); shapes
// beyond lp_batched_two_phase_fits go through lp_simplex_upload + lp_simplex_resolve_run one LP after another
// ===========================================================================

int lp_batched_resolve_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                              const double* c, const int* basis_in, int maximize, int n_orig,
                              lp_batched_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    for (int k = 0; k < batch; ++k) {
        int rc = check_canonical(ctx, A ? A + (size_t)k * m * n : nullptr, m, n,
                                 b ? b + (size_t)k * m : nullptr, c ? c + (size_t)k * n : nullptr,
                                 basis_in ? basis_in + (size_t)k * m : nullptr, n_orig);
        if (rc) return rc;
    }
    LP_HIP(ctx, hipSetDevice(ctx->device));
    lp_batched_problem* p = new lp_batched_problem();
    p->ctx = ctx;
    p->resolve = true;
    p->batch = batch;
    p->m = m;
    p->n = n;
    p->n_orig = n_orig;
    p->maximize = maximize ? 1 : 0;
    const size_t B = (size_t)batch;
    p->status.assign(B, -100);
    p->resolve_iters.assign(B * 2, 0);
    p->h_c.assign(c, c + B * n);
    p->resident = lp_batched_two_phase_fits(m, n);
    if (!p->resident) {   // per-LP fallback: keep the inputs for lp_simplex_resolve_run
        p->h_A.assign(A, A + B * m * n);
        p->h_b.assign(b, b + B * m);
        p->h_basis_in.assign(basis_in, basis_in + B * m);
        p->h_x.assign(B * n_orig, 0.0);
        p->h_obj.assign(B, 0.0);
        p->h_basis.assign(basis_in, basis_in + B * m);
        *problem_out = p;
        return LP_OPTIMAL;
    }
#define LP_TRY(expr)                        \
    do {                                    \
        hipError_t _e = (expr);             \
        if (_e != hipSuccess) {             \
            ctx->last_error = #expr;        \
            lp_batched_free(p);             \
            return -(int)_e;                \
        }                                   \
    } while (0)
    hipStream_t s = ctx->stream;
    LP_TRY(hipMalloc(&p->dA, sizeof(double) * B * m * n));
    LP_TRY(hipMalloc(&p->db, sizeof(double) * B * m));
    LP_TRY(hipMalloc(&p->dc, sizeof(double) * B * n));
    LP_TRY(hipMalloc(&p->dx, sizeof(double) * B * n));
    LP_TRY(hipMalloc(&p->dbasis_in, sizeof(int) * B * m));
    LP_TRY(hipMalloc(&p->dbasis_out, sizeof(int) * B * m));
    LP_TRY(hipMalloc(&p->diters, sizeof(int) * B * 2));
    LP_TRY(hipMalloc(&p->dstatus, sizeof(int) * B));
    LP_TRY(hipEventCreate(&p->ev0));
    LP_TRY(hipEventCreate(&p->ev1));
    LP_TRY(hipMemcpyAsync(p->dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->dbasis_in, basis_in, sizeof(int) * B * m, hipMemcpyHostToDevice, s));
    LP_TRY(hipStreamSynchronize(s));
#undef LP_TRY
    BatchedResolveDev& d = p->rdev;
    d.batch = batch;
    d.m = m;
    d.n = n;
    (void)lp_batched_two_phase_lds_bytes(m, n, &d.pitch);
    d.maximize = p->maximize;
    d.A = p->dA;
    d.b = p->db;
    d.c = p->dc;
    d.basis_in = p->dbasis_in;
    d.x = p->dx;
    d.basis_out = p->dbasis_out;
    d.iters = p->diters;
    d.status = p->dstatus;
    *problem_out = p;
    return LP_OPTIMAL;
}

int lp_batched_set_start(lp_batched_problem* p, const double* b, const int* basis_in) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!p->resolve) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_set_start: not a re-solve batch");
    const size_t B = (size_t)p->batch, m = (size_t)p->m;
    if (basis_in)
        for (size_t k = 0; k < B * m; ++k)
            if (basis_in[k] < 0 || basis_in[k] >= p->n) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    if (!p->resident) {
        if (b) p->h_b.assign(b, b + B * m);
        if (basis_in) p->h_basis_in.assign(basis_in, basis_in + B * m);
        return LP_OPTIMAL;
    }
    LP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (b) LP_HIP(ctx, hipMemcpyAsync(p->db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s));
    if (basis_in) LP_HIP(ctx, hipMemcpyAsync(p->dbasis_in, basis_in, sizeof(int) * B * m, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipStreamSynchronize(s));
    return LP_OPTIMAL;
}

static int batched_resolve_run(lp_batched_problem* p, double eps, int max_iter, float* ms_out) {
    lp_context* ctx = p->ctx;
    if (p->pivot_rule != LP_PIVOT_DANTZIG) LP_FAIL(ctx, LP_BAD_ARG, "the re-solve runs Dantzig's rule only");
    if (p->resident) {
        p->rdev.eps = eps;
        p->rdev.max_iter = max_iter;
        LP_HIP(ctx, hipEventRecord(p->ev0, ctx->stream));
        int rc = lp_batched_resolve_launch(ctx, p->rdev);
        if (rc) return rc;
        LP_HIP(ctx, hipGetLastError());
        LP_HIP(ctx, hipEventRecord(p->ev1, ctx->stream));
        LP_HIP(ctx, hipEventSynchronize(p->ev1));
        float ms = 0.f;
        LP_HIP(ctx, hipEventElapsedTime(&ms, p->ev0, p->ev1));
        if (ms_out) *ms_out = ms;
        return LP_OPTIMAL;
    }
    // per-LP fallback: the single-LP re-solve one LP after another (host clock)
    const auto t0 = std::chrono::steady_clock::now();
    const int m = p->m, n = p->n, no = p->n_orig;
    for (int k = 0; k < p->batch; ++k) {
        lp_simplex_problem* q = nullptr;
        int rc = lp_simplex_upload(ctx, p->h_A.data() + (size_t)k * m * n, m, n, p->h_b.data() + (size_t)k * m,
                                   p->h_c.data() + (size_t)k * n, p->h_basis_in.data() + (size_t)k * m, p->maximize,
                                   no, &q);
        if (rc) return rc;
        rc = lp_simplex_resolve_run(q, eps, max_iter, p->resolve_iters.data() + (size_t)k * 2, nullptr);
        if (rc >= 0) {
            const bool ok = rc == LP_OPTIMAL;
            const int drc = lp_simplex_download(q, ok ? p->h_x.data() + (size_t)k * no : nullptr,
                                                p->h_basis.data() + (size_t)k * m, ok ? p->h_obj.data() + k : nullptr,
                                                nullptr, nullptr, 0, nullptr);
            if (drc) rc = drc;
        }
        lp_simplex_free(q);
        if (rc < 0) return rc;
        p->status[(size_t)k] = rc;
    }
    ctx->last_error.clear();   // (a basis that is no valid start is a per-LP status here)
    if (ms_out) *ms_out = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return LP_OPTIMAL;
}

static int batched_resolve_download(lp_batched_problem* p, double* x_out, int* basis_out, double* obj_out,
                                    int* iters_out, int* status_out) {
    lp_context* ctx = p->ctx;
    const size_t B = (size_t)p->batch;
    const int m = p->m, n = p->n, no = p->n_orig;
    std::vector<double> x;
    if (p->resident) {
        x.resize(B * n);
        hipStream_t s = ctx->stream;
        LP_HIP(ctx, hipMemcpyAsync(x.data(), p->dx, sizeof(double) * B * n, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipMemcpyAsync(p->status.data(), p->dstatus, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipMemcpyAsync(p->resolve_iters.data(), p->diters, sizeof(int) * B * 2, hipMemcpyDeviceToHost, s));
        if (basis_out) LP_HIP(ctx, hipMemcpyAsync(basis_out, p->dbasis_out, sizeof(int) * B * m, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipStreamSynchronize(s));
    } else if (basis_out) {
        std::memcpy(basis_out, p->h_basis.data(), sizeof(int) * B * m);
    }
    for (size_t k = 0; k < B; ++k) {
        const bool ok = p->status[k] == LP_OPTIMAL;
        if (p->resident && ok) {
            const double* xk = x.data() + k * n;
            if (x_out)
                for (int j = 0; j < no; ++j) x_out[k * no + j] = xk[j];
            if (obj_out) {  // Canonical::Evaluate, Canonical.cpp:86
                double z = 0.0;
                const double* ck = p->h_c.data() + k * n;
                for (int j = 0; j < n; ++j) z += ck[j] * xk[j];
                obj_out[k] = z;
            }
        } else if (ok) {
            if (x_out) std::memcpy(x_out + k * no, p->h_x.data() + k * no, sizeof(double) * no);
            if (obj_out) obj_out[k] = p->h_obj[k];
        }
        if (iters_out) iters_out[k] = p->resolve_iters[k * 2] + p->resolve_iters[k * 2 + 1];
        if (status_out) status_out[k] = p->status[k];
    }
    return LP_OPTIMAL;
}

int lp_batched_resolve_iters(lp_batched_problem* p, int* iters_out) {
    if (!p || !iters_out) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!p->resolve) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_resolve_iters: not a re-solve batch");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (p->resident) LP_HIP(ctx, hipMemcpy(p->resolve_iters.data(), p->diters, sizeof(int) * 2 * (size_t)p->batch, hipMemcpyDeviceToHost));
    std::memcpy(iters_out, p->resolve_iters.data(), sizeof(int) * 2 * (size_t)p->batch);
    return LP_OPTIMAL;
}

int lp_simplex_resolve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                               const double* c, const int* basis_in, int maximize, int n_orig, double eps,
                               int max_iter, double* x_out, int* basis_out, double* obj_out, int* iters_out,
                               int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_resolve_batched: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_resolve_batched: eps must be >= 0");
    lp_batched_problem* p = nullptr;
    int rc = lp_batched_resolve_upload(ctx, batch, A, m, n, b, c, basis_in, maximize, n_orig, &p);
    if (rc) return rc;
    rc = lp_batched_run(p, eps, max_iter, nullptr);
    if (rc == LP_OPTIMAL) rc = lp_batched_download(p, x_out, basis_out, obj_out, nullptr, status_out);
    if (rc == LP_OPTIMAL && iters_out) rc = lp_batched_resolve_iters(p, iters_out);
    lp_batched_free(p);
    return rc;
}

int lp_batched_phase_iters(lp_batched_problem* p, int* iters_out) {
    if (!p || !iters_out) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!p->two_phase) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_phase_iters: not a two-phase batch");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (p->resident) LP_HIP(ctx, hipMemcpy(p->phase_iters.data(), p->diters, sizeof(int) * 3 * (size_t)p->batch, hipMemcpyDeviceToHost));
    std::memcpy(iters_out, p->phase_iters.data(), sizeof(int) * 3 * (size_t)p->batch);
    return LP_OPTIMAL;
}

int lp_batched_path(const lp_batched_problem* p) {
    if (!p) return LP_BAD_ARG;
    return p->resident ? 1 : 0;
}

int lp_simplex_two_phase_batched(lp_context* ctx, int batch, const double* A, int m, int n,
                                 const double* b, const double* c, int maximize, int n_orig,
                                 double eps, int max_iter, double* x_out, int* basis_out,
                                 double* obj_out, int* iters_out, int* status_out) {
    return lp_simplex_two_phase_batched_ex(ctx, batch, A, m, n, b, c, maximize, n_orig, eps, max_iter, x_out,
                                           basis_out, obj_out, iters_out, status_out, LP_PIVOT_DANTZIG);
}

int lp_simplex_two_phase_batched_ex(lp_context* ctx, int batch, const double* A, int m, int n,
                                    const double* b, const double* c, int maximize, int n_orig,
                                    double eps, int max_iter, double* x_out, int* basis_out,
                                    double* obj_out, int* iters_out, int* status_out, int pivot_rule) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_two_phase_batched: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_two_phase_batched: eps must be >= 0");
    if (pivot_rule != LP_PIVOT_DANTZIG && pivot_rule != LP_PIVOT_BLAND) LP_FAIL(ctx, LP_BAD_ARG, "unknown pivot rule");
    lp_batched_problem* p = nullptr;
    int rc = lp_batched_two_phase_upload(ctx, batch, A, m, n, b, c, maximize, n_orig, &p);
    if (rc) return rc;
    p->pivot_rule = pivot_rule;
    rc = lp_batched_run(p, eps, max_iter, nullptr);
    if (rc == LP_OPTIMAL) rc = lp_batched_download(p, x_out, basis_out, obj_out, nullptr, status_out);
    if (rc == LP_OPTIMAL && iters_out) rc = lp_batched_phase_iters(p, iters_out);
    lp_batched_free(p);
    return rc;
}

static int batched_run(lp_batched_problem* p, double eps, int max_iter, float* ms_out) {
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (p->two_phase) return batched_two_phase_run(p, eps, max_iter, ms_out);
    if (p->resolve) return batched_resolve_run(p, eps, max_iter, ms_out);
    if (p->resident) {
        p->dev.eps = eps;
        p->dev.max_iter = max_iter;
        if (const char* sv = getenv("LP_BATCHED_STAMPS"); sv && !p->dev.stamps) {   // diagnostic build of the kernel (scripts/stamp_batched.py)
            LP_HIP(ctx, hipMalloc(&p->dev.stamps, sizeof(unsigned long long) * 64));   // 32 phase sums + 2 per wave (16 waves)
            LP_HIP(ctx, hipMemset(p->dev.stamps, 0, sizeof(unsigned long long) * 64));
            p->dev.stamps_reg = std::strcmp(sv, "reg") == 0;
        }
        LP_HIP(ctx, hipEventRecord(p->ev0, ctx->stream));
        int rc = lp_batched_launch(ctx, p->dev, p->pivot_rule);
        if (rc) return rc;
        LP_HIP(ctx, hipEventRecord(p->ev1, ctx->stream));
        LP_HIP(ctx, hipEventSynchronize(p->ev1));
        LP_HIP(ctx, hipGetLastError());
        float ms = 0.f;
        LP_HIP(ctx, hipEventElapsedTime(&ms, p->ev0, p->ev1));
        if (ms_out) *ms_out = ms;
        if (p->dev.stamps) {
            unsigned long long h[64];
            LP_HIP(ctx, hipMemcpy(h, p->dev.stamps, sizeof(h), hipMemcpyDeviceToHost));
            if (p->dev.stamps_reg) {
                fprintf(stderr, "[batched stamps, register form] per wave: pricing | update phase, then the wait at the loop's barrier (incl. the entering column's hand-over):");
                for (int w = 0; w < 8; ++w)
                    fprintf(stderr, "  w%d %.0f+%.0f", w, (double)h[32 + 2 * w] / (double)(h[8] ? h[8] : 1), (double)h[33 + 2 * w] / (double)(h[8] ? h[8] : 1));
                fprintf(stderr, "\n[batched stamps, register form] hand-over per wave:");
                for (int w = 0; w < 8; ++w) fprintf(stderr, "  w%d %.0f", w, (double)h[48 + w] / (double)(h[8] ? h[8] : 1));
                fprintf(stderr, "\n");
                const char* names[8] = {"entering column -> LDS", "barrier", "ratio test | (idle)", "barrier",
                                        "eta column + pivot row -> LDS", "barrier",
                                        "reduced costs + pricing | rank-1 update", "barrier"};
                fprintf(stderr, "[batched stamps, register form] workgroup 0, %llu pivots, %.3f ms: cycles per pivot, wave 0 | wave 1\n", h[8], ms);
                for (int q = 0; q < 8; ++q)
                    fprintf(stderr, "[batched stamps]   %-42s %8.0f | %8.0f\n", names[q], (double)h[q] / (double)(h[8] ? h[8] : 1),
                            (double)h[16 + q] / (double)(h[24] ? h[24] : 1));
            } else {
                const char* names[6] = {"reduced costs + pricing | rank-1 update", "barrier", "ratio test | (idle)", "barrier",
                                        "eta column + pivot-row copy", "barrier"};
                fprintf(stderr, "[batched stamps] workgroup 0, %llu pivots, %.3f ms: cycles per pivot, wave 0 | wave 1\n", h[6], ms);
                for (int q = 0; q < 6; ++q)
                    fprintf(stderr, "[batched stamps]   %-42s %8.0f | %8.0f\n", names[q], (double)h[q] / (double)(h[6] ? h[6] : 1),
                            (double)h[8 + q] / (double)(h[14] ? h[14] : 1));
            }
        }
        return LP_OPTIMAL;
    }
    float total = 0.f;
    for (int k = 0; k < p->batch; ++k) {
        lp_simplex_stats st;
        int rc = lp_simplex_reset(p->lps[(size_t)k]);
        if (rc) return rc;
        p->lps[(size_t)k]->pivot_rule = p->pivot_rule;
        rc = lp_simplex_run(p->lps[(size_t)k], eps, max_iter, LP_SIMPLEX_ALGO_AUTO, &st);
        if (rc < 0) return rc;
        p->status[(size_t)k] = rc;
        p->iters[(size_t)k] = st.pivots;
        total += st.solve_ms;
    }
    if (ms_out) *ms_out = total;
    return LP_OPTIMAL;
}

int lp_batched_run(lp_batched_problem* p, double eps, int max_iter, float* ms_out) {
    if (!p) return LP_BAD_ARG;
    if (!(eps >= 0.0)) LP_FAIL(p->ctx, LP_BAD_ARG, "lp_batched_run: eps must be >= 0");
    const int rc = batched_run(p, eps, max_iter, ms_out);
    p->ran = rc == LP_OPTIMAL;
    return rc;
}

int lp_batched_download(lp_batched_problem* p, double* x_out, int* basis_out, double* obj_out,
                        int* iters_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (p->two_phase) return batched_two_phase_download(p, x_out, basis_out, obj_out, iters_out, status_out);
    if (p->resolve) return batched_resolve_download(p, x_out, basis_out, obj_out, iters_out, status_out);
    if (p->resident) {
        const size_t B = (size_t)p->batch;
        std::vector<double> x(B * p->n);
        hipStream_t s = ctx->stream;
        LP_HIP(ctx, hipMemcpyAsync(x.data(), p->dx, sizeof(double) * B * p->n, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipMemcpyAsync(p->status.data(), p->dstatus, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipMemcpyAsync(p->iters.data(), p->diters, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        if (basis_out)
            LP_HIP(ctx, hipMemcpyAsync(basis_out, p->dbasis_out, sizeof(int) * B * p->m, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipStreamSynchronize(s));
        for (int k = 0; k < p->batch; ++k) {
            const bool ok = p->status[(size_t)k] == LP_OPTIMAL;
            const double* xk = x.data() + (size_t)k * p->n;
            if (x_out && ok)  // x.head(n_orig), SimplexSolover.h:435-438
                for (int j = 0; j < p->n_orig; ++j) x_out[(size_t)k * p->n_orig + j] = xk[j];
            if (obj_out && ok) {  // Canonical::Evaluate, Canonical.cpp:86
                double z = 0.0;
                const double* ck = p->h_c.data() + (size_t)k * p->n;
                for (int j = 0; j < p->n; ++j) z += ck[j] * xk[j];
                obj_out[k] = z;
            }
            if (iters_out) iters_out[k] = p->iters[(size_t)k];
            if (status_out) status_out[k] = p->status[(size_t)k];
        }
        return LP_OPTIMAL;
    }
    for (int k = 0; k < p->batch; ++k) {
        const bool ok = p->status[(size_t)k] == LP_OPTIMAL;
        int rc = lp_simplex_download(p->lps[(size_t)k],
                                     (x_out && ok) ? x_out + (size_t)k * p->n_orig : nullptr,
                                     basis_out ? basis_out + (size_t)k * p->m : nullptr,
                                     (obj_out && ok) ? obj_out + k : nullptr, nullptr, nullptr, 0,
                                     nullptr);
        if (rc) return rc;
        if (iters_out) iters_out[k] = p->iters[(size_t)k];
        if (status_out) status_out[k] = p->status[(size_t)k];
    }
    return LP_OPTIMAL;
}

int lp_simplex_solve_batched(lp_context* ctx, int batch, const double* A, int m, int n,
                             const double* b, const double* c, const int* basis_in, int maximize,
                             int n_orig, double eps, int max_iter, double* x_out, int* basis_out,
                             double* obj_out, int* iters_out, int* status_out) {
    return lp_simplex_solve_batched_ex(ctx, batch, A, m, n, b, c, basis_in, maximize, n_orig, eps, max_iter, x_out,
                                       basis_out, obj_out, iters_out, status_out, LP_PIVOT_DANTZIG);
}

int lp_simplex_solve_batched_ex(lp_context* ctx, int batch, const double* A, int m, int n,
                                const double* b, const double* c, const int* basis_in, int maximize,
                                int n_orig, double eps, int max_iter, double* x_out, int* basis_out,
                                double* obj_out, int* iters_out, int* status_out, int pivot_rule) {
    if (ctx && pivot_rule != LP_PIVOT_DANTZIG && pivot_rule != LP_PIVOT_BLAND)
        LP_FAIL(ctx, LP_BAD_ARG, "unknown pivot rule");
    if (ctx && !(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_solve_batched: eps must be >= 0");
    lp_batched_problem* p = nullptr;
    int rc = lp_batched_upload(ctx, batch, A, m, n, b, c, basis_in, maximize, n_orig, &p);
    if (rc) return rc;
    p->pivot_rule = pivot_rule;
    rc = lp_batched_run(p, eps, max_iter, nullptr);
    if (rc == LP_OPTIMAL) rc = lp_batched_download(p, x_out, basis_out, obj_out, iters_out, status_out);
    lp_batched_free(p);
    return rc;
}

// ===========================================================================
// Bounded-variable simplex (batched_bounded.hip): one LP per workgroup for lp_simplex_bounded_fits shapes only; there
// is no per-LP host fallback
// ===========================================================================

int lp_simplex_bounded_fits(int m, int n) { return lp_bounded_fits_shape(m, n) ? 1 : 0; }

// The checks of both entry points: pointers, dimensions, the bounds of every LP (lo finite, hi not NaN) and the fit.
static int bounded_args(lp_context* ctx, const char* who, int batch, const double* A, int m, int n, const double* b,
                        const double* c, const double* lo, const double* hi, int n_orig) {
    if (!A || !b || !c || !lo || !hi) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (m <= 0 || n < m || n_orig <= 0 || n_orig > n) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    const size_t N = (size_t)batch * n;
    for (size_t j = 0; j < N; ++j) {
        if (!std::isfinite(lo[j])) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": lo must be finite");
        if (std::isnan(hi[j])) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": hi is NaN");
    }
    if (!lp_bounded_fits_shape(m, n))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the shape does not fit one CU's LDS (lp_simplex_bounded_fits)");
    return LP_OPTIMAL;
}

// Uploads `batch` LPs, runs k_batched_bounded and downloads; x (n_orig) and obj (over all n columns, as
// lp_simplex_two_phase_batched) are written for LP_OPTIMAL LPs only.
static int bounded_solve(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                         const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter,
                         double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out,
                         int* status_out) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch;
    const size_t dbl = B * ((size_t)m * n + m + 4 * (size_t)n), ints = B * ((size_t)m + n + 4 + 1);
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * dbl + sizeof(int) * ints));
    BatchedBoundedDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    (void)lp_bounded_lds_bytes(m, n, &d.pitch);
    d.maximize = maximize ? 1 : 0;
    d.max_iter = max_iter;
    d.eps = eps;
    double* dA = reinterpret_cast<double*>(buf.ptr);
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    double* dlo = dc + B * n;
    double* dhi = dlo + B * n;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.lo = dlo;
    d.hi = dhi;
    d.x = dhi + B * n;
    d.basis_out = reinterpret_cast<int*>(d.x + B * n);
    d.at_upper = d.basis_out + B * m;
    d.iters = d.at_upper + B * n;
    d.status = d.iters + B * 4;
    std::vector<double> x(B * n);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dlo, lo, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dhi, hi, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched bounded simplex upload: ") + hipGetErrorString(e));
    int rc = lp_batched_bounded_launch(ctx, d);
    if (rc) return rc;
    e = hipGetLastError();
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched bounded simplex: ") + hipGetErrorString(e));
    rc = lp_download(ctx, "batched bounded simplex", {{x.data(), d.x, sizeof(double) * B * n},
                                                      {basis_out, d.basis_out, sizeof(int) * B * m},
                                                      {at_upper_out, d.at_upper, sizeof(int) * B * n},
                                                      {iters_out, d.iters, sizeof(int) * B * 4},
                                                      {status_out, d.status, sizeof(int) * B}});
    if (rc) return rc;
    for (size_t k = 0; k < B; ++k) {
        if (status_out[k] != LP_OPTIMAL) continue;
        const double* xk = x.data() + k * n;
        for (int j = 0; j < n_orig; ++j) x_out[k * n_orig + j] = xk[j];
        double z = 0.0;   // Canonical::Evaluate, Canonical.cpp:86
        const double* ck = c + k * n;
        for (int j = 0; j < n; ++j) z += ck[j] * xk[j];
        obj_out[k] = z;
    }
    return LP_OPTIMAL;
}

int lp_simplex_bounded(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                       const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter,
                       double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out || !basis_out || !at_upper_out || !obj_out || !iters_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_bounded: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_bounded: eps must be >= 0");
    int rc = bounded_args(ctx, "lp_simplex_bounded", 1, A, m, n, b, c, lo, hi, n_orig);
    if (rc) return rc;
    int status = LP_OPTIMAL;
    rc = bounded_solve(ctx, 1, A, m, n, b, c, lo, hi, maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out,
                       obj_out, iters_out, &status);
    return rc ? rc : status;
}

int lp_simplex_bounded_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                               const double* c, const double* lo, const double* hi, int maximize, int n_orig,
                               double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out,
                               double* obj_out, int* iters_out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out || !basis_out || !at_upper_out || !obj_out || !iters_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_bounded_batched: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_bounded_batched: eps must be >= 0");
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    const int rc = bounded_args(ctx, "lp_simplex_bounded_batched", batch, A, m, n, b, c, lo, hi, n_orig);
    if (rc) return rc;
    return bounded_solve(ctx, batch, A, m, n, b, c, lo, hi, maximize, n_orig, eps, max_iter, x_out, basis_out,
                         at_upper_out, obj_out, iters_out, status_out);
}

}  // extern "C"
