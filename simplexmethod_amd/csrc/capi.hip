// capi.hip — the extern "C" boundary (include/simplexmethod_amd.h): the context, the status strings, the
// division self-tests and the batched simplex.  The single-LP simplex is simplex_driver.hip, the
// enumeration enum_driver.hip.
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

struct lp_batched_problem {
    lp_context* ctx = nullptr;
    int batch = 0, m = 0, n = 0, n_orig = 0;
    bool resident = false;              // true: LDS-resident kernel; false: per-LP fallback
    BatchedDev dev{};
    double *dA = nullptr, *db = nullptr, *dc = nullptr, *dx = nullptr;
    int *dbasis_in = nullptr, *dbasis_out = nullptr, *diters = nullptr, *dstatus = nullptr;
    std::vector<double> h_c;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<lp_simplex_problem*> lps;  // fallback
    std::vector<int> status, iters;
    // two-phase batch (lp_batched_two_phase_upload): no basis_in, three pivot counts per LP
    bool two_phase = false;
    int maximize = 0;
    BatchedTwoPhaseDev tdev{};
    std::vector<int> phase_iters;           // batch*3
    std::vector<double> h_A, h_b;           // per-LP fallback: the inputs ...
    std::vector<double> h_x, h_obj;         // ... and its outputs (x batch*n_orig, obj batch)
    std::vector<int> h_basis;               // batch*m
    int pivot_rule = LP_PIVOT_DANTZIG;      // lp_batched_set_pivot_rule: read by every run
    // re-solve batch (lp_batched_resolve_upload): given bases, two pivot counts per LP; the per-LP fallback keeps
    // h_A, h_b, h_basis_in and its outputs in h_x, h_obj, h_basis
    bool resolve = false;
    BatchedResolveDev rdev{};
    std::vector<int> resolve_iters;         // batch*2: dual, primal
    std::vector<int> h_basis_in;            // batch*m
    bool ran = false;                       // a run completed: lp_batched_duals / _ranging / _certificates have final bases to read
};

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
// the dual solution at a given basis (basis_duals.hip): one LP per workgroup for lp_basis_duals_fits(m), the
// single-LP launch pair one LP after another beyond it
// ===========================================================================

int lp_basis_duals_fits(int m) { return m > 0 && lp_basis_duals_lds_bytes(m) <= 160 * 1024 ? 1 : 0; }

// Duals of `batch` LPs whose inputs are on the device; drun_status (device, or nullptr): LPs whose run status is
// not LP_OPTIMAL keep it and get NaN.  Outputs to the host.
static int duals_on_device(lp_context* ctx, int batch, int m, int n, const double* dA, const double* db,
                           const double* dc, const int* dbasis, const int* drun_status, double* y_out, double* d_out,
                           double* w_out, int* status_out) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch;
    const size_t bytes = sizeof(double) * B * ((size_t)m + n + 1) + sizeof(int) * B;
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, bytes));
    BasisDualsDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.basis = dbasis;
    d.run_status = drun_status;
    d.y = reinterpret_cast<double*>(buf);
    d.d = d.y + B * m;
    d.w = d.d + B * n;
    d.status = reinterpret_cast<int*>(d.w + B);
    int rc = LP_OPTIMAL;
    if (lp_basis_duals_fits(m)) {
        rc = lp_basis_duals_launch(ctx, d);
    } else {   // one LP after another: statuses and bases checked on the host
        std::vector<int> st(B, LP_OPTIMAL), basis(B * m);
        hipError_t e = hipMemcpyAsync(basis.data(), dbasis, sizeof(int) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && drun_status)
            e = hipMemcpyAsync(st.data(), drun_status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(buf);
            LP_HIP(ctx, e);
        }
        for (size_t k = 0; k < B && rc >= 0; ++k) {
            if (st[k] == LP_OPTIMAL)
                for (int t = 0; t < m; ++t)
                    if (basis[k * m + t] < 0 || basis[k * m + t] >= n) st[k] = LP_BAD_ARG;
            if (st[k] != LP_OPTIMAL) continue;
            rc = lp_basis_duals_device(ctx, dA + k * m * n, m, n, db + k * m, dc + k * n, dbasis + k * m,
                                       d.y + k * m, d.d + k * n, d.w + k);
            if (rc >= 0) st[k] = rc;
        }
        if (rc >= 0) {
            rc = LP_OPTIMAL;
            e = hipMemcpyAsync(d.status, st.data(), sizeof(int) * B, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = -(int)e;
        }
    }
    if (rc == LP_OPTIMAL) {
        hipError_t e = hipMemcpyAsync(y_out, d.y, sizeof(double) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_out, d.d, sizeof(double) * B * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(w_out, d.w, sizeof(double) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(status_out, d.status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ctx->last_error = std::string("basis duals: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(buf);
    if (rc != LP_OPTIMAL) return rc;
    // LPs without duals: NaN (the per-LP path leaves their outputs unwritten)
    for (size_t k = 0; k < B; ++k) {
        if (status_out[k] == LP_OPTIMAL) continue;
        for (int t = 0; t < m; ++t) y_out[k * m + t] = NAN;
        for (int j = 0; j < n; ++j) d_out[k * n + j] = NAN;
        w_out[k] = NAN;
    }
    return LP_OPTIMAL;
}

// Uploads `batch` LPs, then duals_on_device.
static int duals_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                        const int* basis, double* y_out, double* d_out, double* w_out, int* status_out) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, dbl = B * ((size_t)m * n + m + n);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, sizeof(double) * dbl + sizeof(int) * B * m));
    double* dA = reinterpret_cast<double*>(buf);
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    int* dbasis = reinterpret_cast<int*>(dc + B * n);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    int rc = LP_OPTIMAL;
    if (e != hipSuccess) {
        ctx->last_error = std::string("basis duals upload: ") + hipGetErrorString(e);
        rc = -(int)e;
    } else {
        rc = duals_on_device(ctx, batch, m, n, dA, db, dc, dbasis, nullptr, y_out, d_out, w_out, status_out);
    }
    (void)hipFree(buf);
    return rc;
}

int lp_basis_duals(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                   const int* basis, double* y_out, double* d_out, double* w_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !y_out || !d_out || !w_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_duals: null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_duals: bad dimensions");
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    int status = LP_OPTIMAL;
    const int rc = duals_upload(ctx, 1, A, m, n, b, c, basis, y_out, d_out, w_out, &status);
    return rc ? rc : status;
}

int lp_basis_duals_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                           const double* c, const int* basis, double* y_out, double* d_out, double* w_out,
                           int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !y_out || !d_out || !w_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_duals_batched: null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_duals_batched: bad dimensions");
    return duals_upload(ctx, batch, A, m, n, b, c, basis, y_out, d_out, w_out, status_out);
}

int lp_batched_duals(lp_batched_problem* p, double* y_out, double* d_out, double* w_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!y_out || !d_out || !w_out || !status_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_duals: null argument");
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_duals: the batch has not run");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const int m = p->m, n = p->n;
    if (p->resident)   // A, b, c, the final bases and the run statuses where the run left them
        return duals_on_device(ctx, p->batch, m, n, p->dA, p->db, p->dc, p->dbasis_out, p->dstatus, y_out, d_out,
                               w_out, status_out);
    // per-LP fallback: the single-LP call on the kept inputs and each LP's final basis
    std::vector<int> basis((size_t)m);
    for (size_t k = 0; k < (size_t)p->batch; ++k) {
        double* y = y_out + k * m;
        double* d = d_out + k * n;
        int st = p->status[k];
        if (st == LP_OPTIMAL) {
            if (p->two_phase || p->resolve) {
                std::memcpy(basis.data(), p->h_basis.data() + k * m, sizeof(int) * m);
            } else {
                const int rc = lp_simplex_download(p->lps[k], nullptr, basis.data(), nullptr, nullptr, nullptr, 0, nullptr);
                if (rc) return rc;
            }
            st = lp_basis_duals(ctx, p->h_A.data() + k * m * n, m, n, p->h_b.data() + k * m, p->h_c.data() + k * n,
                                basis.data(), y, d, w_out + k);
            if (st < 0) return st;
        }
        status_out[k] = st;
        if (st != LP_OPTIMAL) {
            for (int t = 0; t < m; ++t) y[t] = NAN;
            for (int j = 0; j < n; ++j) d[j] = NAN;
            w_out[k] = NAN;
        }
    }
    ctx->last_error.clear();
    return LP_OPTIMAL;
}

// ===========================================================================
// RHS and cost ranging at a given basis (basis_ranging.hip): one LP per workgroup for lp_basis_ranging_fits(m, n),
// the single-LP path one LP after another beyond it
// ===========================================================================

int lp_basis_ranging_fits(int m, int n) {
    return m > 0 && n >= m && lp_basis_ranging_lds_bytes(m, n) <= 160 * 1024 ? 1 : 0;
}

// NaN values and -1 indices for LP k
static void ranging_nan(size_t k, int m, int n, double* rhs, int* rhs_var, double* cost, int* cost_var) {
    for (size_t q = 0; q < 2 * (size_t)m; ++q) {
        rhs[k * 2 * m + q] = NAN;
        rhs_var[k * 2 * m + q] = -1;
    }
    for (size_t q = 0; q < 2 * (size_t)n; ++q) {
        cost[k * 2 * n + q] = NAN;
        cost_var[k * 2 * n + q] = -1;
    }
}

// Ranges of `batch` LPs whose inputs are on the device; drun_status (device, or nullptr): LPs whose run status is
// not LP_OPTIMAL keep it and get NaN.  Outputs to the host.
static int ranging_on_device(lp_context* ctx, int batch, int m, int n, const double* dA, const double* db,
                             const double* dc, const int* dbasis, const int* drun_status, int maximize, double eps,
                             double* rhs_out, int* rhs_var_out, double* cost_out, int* cost_var_out,
                             int* status_out) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch, nr = B * 2 * m, nc = B * 2 * n;
    const size_t bytes = sizeof(double) * (nr + nc) + sizeof(int) * (nr + nc + B);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, bytes));
    BasisRangingDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.maximize = maximize ? 1 : 0;
    d.eps = eps;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.basis = dbasis;
    d.run_status = drun_status;
    d.rhs = reinterpret_cast<double*>(buf);
    d.cost = d.rhs + nr;
    d.rhs_var = reinterpret_cast<int*>(d.cost + nc);
    d.cost_var = d.rhs_var + nr;
    d.status = d.cost_var + nc;
    int rc = LP_OPTIMAL;
    if (lp_basis_ranging_fits(m, n)) {
        rc = lp_basis_ranging_launch(ctx, d);
    } else {   // one LP after another: statuses and bases checked on the host
        std::vector<int> st(B, LP_OPTIMAL), basis(B * m);
        hipError_t e = hipMemcpyAsync(basis.data(), dbasis, sizeof(int) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && drun_status)
            e = hipMemcpyAsync(st.data(), drun_status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(buf);
            LP_HIP(ctx, e);
        }
        for (size_t k = 0; k < B && rc >= 0; ++k) {
            if (st[k] == LP_OPTIMAL)
                for (int t = 0; t < m; ++t)
                    if (basis[k * m + t] < 0 || basis[k * m + t] >= n) st[k] = LP_BAD_ARG;
            if (st[k] != LP_OPTIMAL) continue;
            rc = lp_basis_ranging_device(ctx, dA + k * m * n, m, n, db + k * m, dc + k * n, dbasis + k * m,
                                         d.maximize, eps, d.rhs + k * 2 * m, d.rhs_var + k * 2 * m,
                                         d.cost + k * 2 * n, d.cost_var + k * 2 * n);
            if (rc >= 0) st[k] = rc;
        }
        if (rc >= 0) {
            rc = LP_OPTIMAL;
            e = hipMemcpyAsync(d.status, st.data(), sizeof(int) * B, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = -(int)e;
        }
    }
    if (rc == LP_OPTIMAL) {
        hipError_t e = hipMemcpyAsync(rhs_out, d.rhs, sizeof(double) * nr, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(rhs_var_out, d.rhs_var, sizeof(int) * nr, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(cost_out, d.cost, sizeof(double) * nc, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(cost_var_out, d.cost_var, sizeof(int) * nc, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(status_out, d.status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ctx->last_error = std::string("basis ranging: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(buf);
    if (rc != LP_OPTIMAL) return rc;
    // LPs without ranges: NaN (the per-LP path leaves their outputs unwritten)
    for (size_t k = 0; k < B; ++k)
        if (status_out[k] != LP_OPTIMAL) ranging_nan(k, m, n, rhs_out, rhs_var_out, cost_out, cost_var_out);
    return LP_OPTIMAL;
}

// Uploads `batch` LPs, then ranging_on_device.
static int ranging_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                          const int* basis, int maximize, double eps, double* rhs_out, int* rhs_var_out,
                          double* cost_out, int* cost_var_out, int* status_out) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, dbl = B * ((size_t)m * n + m + n);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, sizeof(double) * dbl + sizeof(int) * B * m));
    double* dA = reinterpret_cast<double*>(buf);
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    int* dbasis = reinterpret_cast<int*>(dc + B * n);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    int rc = LP_OPTIMAL;
    if (e != hipSuccess) {
        ctx->last_error = std::string("basis ranging upload: ") + hipGetErrorString(e);
        rc = -(int)e;
    } else {
        rc = ranging_on_device(ctx, batch, m, n, dA, db, dc, dbasis, nullptr, maximize, eps, rhs_out, rhs_var_out,
                               cost_out, cost_var_out, status_out);
    }
    (void)hipFree(buf);
    return rc;
}

int lp_basis_ranging(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                     const int* basis, int maximize, double eps, double* rhs_out, int* rhs_var_out,
                     double* cost_out, int* cost_var_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !rhs_out || !rhs_var_out || !cost_out || !cost_var_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_ranging: null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_ranging: bad dimensions");
    ranging_nan(0, m, n, rhs_out, rhs_var_out, cost_out, cost_var_out);
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_ranging: eps must be >= 0");
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    int status = LP_OPTIMAL;
    const int rc = ranging_upload(ctx, 1, A, m, n, b, c, basis, maximize, eps, rhs_out, rhs_var_out, cost_out,
                                  cost_var_out, &status);
    return rc ? rc : status;
}

int lp_basis_ranging_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                             const double* c, const int* basis, int maximize, double eps, double* rhs_out,
                             int* rhs_var_out, double* cost_out, int* cost_var_out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !rhs_out || !rhs_var_out || !cost_out || !cost_var_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_ranging_batched: null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_ranging_batched: bad dimensions");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_ranging_batched: eps must be >= 0");
    return ranging_upload(ctx, batch, A, m, n, b, c, basis, maximize, eps, rhs_out, rhs_var_out, cost_out,
                          cost_var_out, status_out);
}

int lp_batched_ranging(lp_batched_problem* p, double eps, double* rhs_out, int* rhs_var_out, double* cost_out,
                       int* cost_var_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!rhs_out || !rhs_var_out || !cost_out || !cost_var_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_ranging: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_ranging: eps must be >= 0");
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_ranging: the batch has not run");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const int m = p->m, n = p->n;
    if (p->resident)   // A, b, c, the final bases and the run statuses where the run left them
        return ranging_on_device(ctx, p->batch, m, n, p->dA, p->db, p->dc, p->dbasis_out, p->dstatus, p->maximize,
                                 eps, rhs_out, rhs_var_out, cost_out, cost_var_out, status_out);
    // per-LP fallback: the single-LP call on the kept inputs and each LP's final basis
    std::vector<int> basis((size_t)m);
    for (size_t k = 0; k < (size_t)p->batch; ++k) {
        int st = p->status[k];
        if (st == LP_OPTIMAL) {
            if (p->two_phase || p->resolve) {
                std::memcpy(basis.data(), p->h_basis.data() + k * m, sizeof(int) * m);
            } else {
                const int rc = lp_simplex_download(p->lps[k], nullptr, basis.data(), nullptr, nullptr, nullptr, 0, nullptr);
                if (rc) return rc;
            }
            st = lp_basis_ranging(ctx, p->h_A.data() + k * m * n, m, n, p->h_b.data() + k * m, p->h_c.data() + k * n,
                                  basis.data(), p->maximize, eps, rhs_out + k * 2 * m, rhs_var_out + k * 2 * m,
                                  cost_out + k * 2 * n, cost_var_out + k * 2 * n);
            if (st < 0) return st;
        }
        status_out[k] = st;
        if (st != LP_OPTIMAL) ranging_nan(k, m, n, rhs_out, rhs_var_out, cost_out, cost_var_out);
    }
    ctx->last_error.clear();
    return LP_OPTIMAL;
}

// ===========================================================================
// Farkas and unbounded-ray certificates at a given basis (basis_certificate.hip): one LP per workgroup for
// lp_basis_certificate_fits(m, n), the single-LP path one LP after another beyond it
// ===========================================================================

int lp_basis_certificate_fits(int m, int n) {
    return m > 0 && n > 0 && lp_basis_certificate_lds_bytes(m, n) <= 160 * 1024 ? 1 : 0;
}

// NONE, NaN values and index -1 for LP k
static void certificate_none(size_t k, int m, int n, int* kind, double* farkas, double* ray, double* value,
                             int* index) {
    kind[k] = LP_CERT_NONE;
    for (size_t q = 0; q < (size_t)m; ++q) farkas[k * m + q] = NAN;
    for (size_t q = 0; q < (size_t)n; ++q) ray[k * n + q] = NAN;
    value[k] = NAN;
    index[k] = -1;
}

// The basis check of one LP on the host: LP_BAD_ARG (an index outside [0, n+m)), LP_SINGULAR (a repeat), else
// LP_OPTIMAL.
static int certificate_basis_check(const int* basis, int m, int n) {
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n + m) return LP_BAD_ARG;
    std::vector<char> seen((size_t)n + m, 0);
    for (int t = 0; t < m; ++t) {
        if (seen[(size_t)basis[t]]) return LP_SINGULAR;
        seen[(size_t)basis[t]] = 1;
    }
    return LP_OPTIMAL;
}

// Certificates of `batch` LPs whose inputs are on the device; drun_status (device, or nullptr): only LPs whose run
// status is LP_INFEASIBLE / LP_UNBOUNDED get one, the others keep it and get NONE.  Outputs to the host.
static int certificate_on_device(lp_context* ctx, int batch, int m, int n, const double* dA, const double* db,
                                 const double* dc, const int* dbasis, const int* drun_status, int maximize,
                                 double eps, int* kind_out, double* farkas_out, double* ray_out, double* value_out,
                                 int* index_out, int* status_out) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch, nf = B * m, nr = B * n;
    const size_t bytes = sizeof(double) * (nf + nr + B) + sizeof(int) * 3 * B;
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, bytes));
    BasisCertificateDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.maximize = maximize ? 1 : 0;
    d.eps = eps;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.basis = dbasis;
    d.run_status = drun_status;
    d.farkas = reinterpret_cast<double*>(buf);
    d.ray = d.farkas + nf;
    d.value = d.ray + nr;
    d.kind = reinterpret_cast<int*>(d.value + B);
    d.index = d.kind + B;
    d.status = d.index + B;
    std::vector<char> done(B, 1);   // the LP's outputs were written on the device
    int rc = LP_OPTIMAL;
    if (lp_basis_certificate_fits(m, n)) {
        rc = lp_basis_certificate_launch(ctx, d);
    } else {   // one LP after another: statuses and bases checked on the host
        std::vector<int> st(B, LP_OPTIMAL), basis(B * m);
        hipError_t e = hipMemcpyAsync(basis.data(), dbasis, sizeof(int) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && drun_status)
            e = hipMemcpyAsync(st.data(), drun_status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(buf);
            LP_HIP(ctx, e);
        }
        for (size_t k = 0; k < B && rc >= 0; ++k) {
            done[k] = 0;
            if (drun_status && st[k] != LP_INFEASIBLE && st[k] != LP_UNBOUNDED) continue;
            int cs = certificate_basis_check(basis.data() + k * m, m, n);
            if (cs == LP_OPTIMAL) {
                rc = lp_basis_certificate_device(ctx, dA + k * m * n, m, n, db + k * m, dc + k * n, dbasis + k * m,
                                                 d.maximize, eps, d.kind + k, d.farkas + k * m, d.ray + k * n,
                                                 d.value + k, d.index + k);
                if (rc < 0) break;
                cs = rc;
                done[k] = cs == LP_OPTIMAL;
            }
            if (cs != LP_OPTIMAL) st[k] = cs;
        }
        if (rc >= 0) {
            rc = LP_OPTIMAL;
            e = hipMemcpyAsync(d.status, st.data(), sizeof(int) * B, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = -(int)e;
        }
    }
    if (rc == LP_OPTIMAL) {
        hipError_t e = hipMemcpyAsync(farkas_out, d.farkas, sizeof(double) * nf, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(ray_out, d.ray, sizeof(double) * nr, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(value_out, d.value, sizeof(double) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(kind_out, d.kind, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(index_out, d.index, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(status_out, d.status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ctx->last_error = std::string("basis certificate: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(buf);
    if (rc != LP_OPTIMAL) return rc;
    // LPs without a certificate on the per-LP path: NONE (their outputs were left unwritten)
    for (size_t k = 0; k < B; ++k)
        if (!done[k]) certificate_none(k, m, n, kind_out, farkas_out, ray_out, value_out, index_out);
    return LP_OPTIMAL;
}

// Uploads `batch` LPs, then certificate_on_device.
static int certificate_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                              const double* c, const int* basis, int maximize, double eps, int* kind_out,
                              double* farkas_out, double* ray_out, double* value_out, int* index_out,
                              int* status_out) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, dbl = B * ((size_t)m * n + m + n);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, sizeof(double) * dbl + sizeof(int) * B * m));
    double* dA = reinterpret_cast<double*>(buf);
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    int* dbasis = reinterpret_cast<int*>(dc + B * n);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    int rc = LP_OPTIMAL;
    if (e != hipSuccess) {
        ctx->last_error = std::string("basis certificate upload: ") + hipGetErrorString(e);
        rc = -(int)e;
    } else {
        rc = certificate_on_device(ctx, batch, m, n, dA, db, dc, dbasis, nullptr, maximize, eps, kind_out,
                                   farkas_out, ray_out, value_out, index_out, status_out);
    }
    (void)hipFree(buf);
    return rc;
}

int lp_basis_certificate(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                         const int* basis, int maximize, double eps, int* kind_out, double* farkas_out,
                         double* ray_out, double* value_out, int* index_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !kind_out || !farkas_out || !ray_out || !value_out || !index_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_certificate: null argument");
    if (m <= 0 || n <= 0) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_certificate: bad dimensions");
    certificate_none(0, m, n, kind_out, farkas_out, ray_out, value_out, index_out);
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_certificate: eps must be >= 0");
    const int cs = certificate_basis_check(basis, m, n);
    if (cs == LP_BAD_ARG) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    if (cs == LP_SINGULAR) return LP_SINGULAR;
    int status = LP_OPTIMAL;
    const int rc = certificate_upload(ctx, 1, A, m, n, b, c, basis, maximize, eps, kind_out, farkas_out, ray_out,
                                      value_out, index_out, &status);
    return rc ? rc : status;
}

int lp_basis_certificate_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                 const double* c, const int* basis, int maximize, double eps, int* kind_out,
                                 double* farkas_out, double* ray_out, double* value_out, int* index_out,
                                 int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !kind_out || !farkas_out || !ray_out || !value_out || !index_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_certificate_batched: null argument");
    if (batch <= 0 || m <= 0 || n <= 0) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_certificate_batched: bad dimensions");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_certificate_batched: eps must be >= 0");
    return certificate_upload(ctx, batch, A, m, n, b, c, basis, maximize, eps, kind_out, farkas_out, ray_out,
                              value_out, index_out, status_out);
}

int lp_batched_certificates(lp_batched_problem* p, double eps, int* kind_out, double* farkas_out, double* ray_out,
                            double* value_out, int* index_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!kind_out || !farkas_out || !ray_out || !value_out || !index_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_certificates: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_certificates: eps must be >= 0");
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_certificates: the batch has not run");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const int m = p->m, n = p->n;
    if (p->resident)   // A, b, c, the final bases and the run statuses where the run left them
        return certificate_on_device(ctx, p->batch, m, n, p->dA, p->db, p->dc, p->dbasis_out, p->dstatus,
                                     p->maximize, eps, kind_out, farkas_out, ray_out, value_out, index_out,
                                     status_out);
    // per-LP fallback: the single-LP call on the kept inputs and each LP's final basis
    std::vector<int> basis((size_t)m);
    for (size_t k = 0; k < (size_t)p->batch; ++k) {
        int st = p->status[k];
        certificate_none(k, m, n, kind_out, farkas_out, ray_out, value_out, index_out);
        if (st == LP_INFEASIBLE || st == LP_UNBOUNDED) {
            if (p->two_phase || p->resolve) {
                std::memcpy(basis.data(), p->h_basis.data() + k * m, sizeof(int) * m);
            } else {
                const int rc = lp_simplex_download(p->lps[k], nullptr, basis.data(), nullptr, nullptr, nullptr, 0, nullptr);
                if (rc) return rc;
            }
            const int cs = lp_basis_certificate(ctx, p->h_A.data() + k * m * n, m, n, p->h_b.data() + k * m,
                                                p->h_c.data() + k * n, basis.data(), p->maximize, eps, kind_out + k,
                                                farkas_out + k * m, ray_out + k * n, value_out + k, index_out + k);
            if (cs < 0) return cs;
            if (cs != LP_OPTIMAL) st = cs;
        }
        status_out[k] = st;
    }
    ctx->last_error.clear();
    return LP_OPTIMAL;
}

// ===========================================================================
// Parametric right-hand side from an optimal basis (basis_parametric.hip): one LP per workgroup for
// lp_basis_parametric_fits(m, n), the single-LP launch path one LP after another beyond it
// ===========================================================================

int lp_basis_parametric_fits(int m, int n) {
    return m > 0 && n >= m && lp_basis_parametric_lds_bytes(m, n, nullptr) <= 160 * 1024 ? 1 : 0;
}

// LP k without a path: nseg 0, NaN / -1, the given basis (host) back
static void parametric_none(size_t k, int m, int mb, const int* basis, int* nseg, double* t, double* obj,
                            double* slope, int* enter, int* leave, int* basis_out) {
    nseg[k] = 0;
    for (size_t q = 0; q < (size_t)mb + 2; ++q) {
        t[k * (mb + 2) + q] = NAN;
        obj[k * (mb + 2) + q] = NAN;
    }
    for (size_t q = 0; q < (size_t)mb + 1; ++q) {
        slope[k * (mb + 1) + q] = NAN;
        enter[k * (mb + 1) + q] = -1;
        leave[k * (mb + 1) + q] = -1;
    }
    if (basis) std::memcpy(basis_out + k * m, basis, sizeof(int) * (size_t)m);
}

// Paths of `batch` LPs whose inputs (d included) are on the device; drun_status (device, or nullptr): LPs whose run
// status is not LP_OPTIMAL keep it and get nseg 0.  Outputs to the host.
static int parametric_on_device(lp_context* ctx, int batch, int m, int n, const double* dA, const double* db,
                                const double* dc, const int* dbasis, const int* drun_status, const double* ddir,
                                int maximize, double t_max, double eps, int mb, int* nseg_out, double* t_out,
                                double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* basis_out,
                                int* status_out) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch, nt = B * (mb + 2), ns = B * (mb + 1);
    const size_t bytes = sizeof(double) * (2 * nt + ns) + sizeof(int) * (2 * ns + B * m + 2 * B);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, bytes));
    BasisParametricDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    (void)lp_basis_parametric_lds_bytes(m, n, &d.pitch);
    d.max_breaks = mb;
    d.eps = eps;
    d.t_max = t_max;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.dir = ddir;
    d.basis = dbasis;
    d.run_status = drun_status;
    d.t = reinterpret_cast<double*>(buf);
    d.obj = d.t + nt;
    d.slope = d.obj + nt;
    d.enter = reinterpret_cast<int*>(d.slope + ns);
    d.leave = d.enter + ns;
    d.basis_out = d.leave + ns;
    d.nseg = d.basis_out + B * m;
    d.status = d.nseg + B;
    std::vector<char> done(B, 1);   // the LP's outputs were written on the device
    std::vector<int> basis;         // per-LP path: the given bases
    int rc = LP_OPTIMAL;
    if (lp_basis_parametric_fits(m, n)) {
        rc = lp_basis_parametric_launch(ctx, d, maximize);
    } else {   // one LP after another: statuses and bases checked on the host
        std::vector<int> st(B, LP_OPTIMAL);
        basis.resize(B * m);
        hipError_t e = hipMemcpyAsync(basis.data(), dbasis, sizeof(int) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && drun_status)
            e = hipMemcpyAsync(st.data(), drun_status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(buf);
            LP_HIP(ctx, e);
        }
        for (size_t k = 0; k < B && rc >= 0; ++k) {
            done[k] = 0;
            if (st[k] != LP_OPTIMAL) continue;
            for (int t = 0; t < m; ++t)
                if (basis[k * m + t] < 0 || basis[k * m + t] >= n) st[k] = LP_BAD_ARG;
            if (st[k] != LP_OPTIMAL) continue;
            rc = lp_basis_parametric_device(ctx, dA + k * m * n, m, n, db + k * m, dc + k * n, dbasis + k * m,
                                            ddir + k * m, maximize, t_max, eps, mb, d.nseg + k, d.t + k * (mb + 2),
                                            d.obj + k * (mb + 2), d.slope + k * (mb + 1), d.enter + k * (mb + 1),
                                            d.leave + k * (mb + 1), d.basis_out + k * m);
            if (rc < 0) break;
            st[k] = rc;
            done[k] = rc == LP_OPTIMAL || rc == LP_INFEASIBLE || rc == LP_ITER_LIMIT;
        }
        if (rc >= 0) {
            rc = LP_OPTIMAL;
            e = hipMemcpyAsync(d.status, st.data(), sizeof(int) * B, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = -(int)e;
        }
    }
    if (rc == LP_OPTIMAL) {
        hipError_t e = hipMemcpyAsync(t_out, d.t, sizeof(double) * nt, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(obj_out, d.obj, sizeof(double) * nt, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(slope_out, d.slope, sizeof(double) * ns, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(enter_out, d.enter, sizeof(int) * ns, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(leave_out, d.leave, sizeof(int) * ns, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(basis_out, d.basis_out, sizeof(int) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nseg_out, d.nseg, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(status_out, d.status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ctx->last_error = std::string("basis parametric: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(buf);
    if (rc != LP_OPTIMAL) return rc;
    if (!basis.empty())   // the per-LP path writes the path only: the rest is NaN / -1, and LPs without one get it all
        for (size_t k = 0; k < B; ++k) {
            if (!done[k]) {
                parametric_none(k, m, mb, basis.data() + k * m, nseg_out, t_out, obj_out, slope_out, enter_out,
                                leave_out, basis_out);
                continue;
            }
            const int ns_k = nseg_out[k];
            for (int q = ns_k + 1; q < mb + 2; ++q) t_out[k * (mb + 2) + q] = obj_out[k * (mb + 2) + q] = NAN;
            for (int q = ns_k; q < mb + 1; ++q) {
                slope_out[k * (mb + 1) + q] = NAN;
                enter_out[k * (mb + 1) + q] = leave_out[k * (mb + 1) + q] = -1;
            }
        }
    return LP_OPTIMAL;
}

// Uploads `batch` LPs and their directions, then parametric_on_device.
static int parametric_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                             const double* c, const int* basis, int maximize, const double* dir, double t_max,
                             double eps, int mb, int* nseg_out, double* t_out, double* obj_out, double* slope_out,
                             int* enter_out, int* leave_out, int* basis_out, int* status_out) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, dbl = B * ((size_t)m * n + 2 * m + n);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, sizeof(double) * dbl + sizeof(int) * B * m));
    double* dA = reinterpret_cast<double*>(buf);
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    double* ddir = dc + B * n;
    int* dbasis = reinterpret_cast<int*>(ddir + B * m);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ddir, dir, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    int rc = LP_OPTIMAL;
    if (e != hipSuccess) {
        ctx->last_error = std::string("basis parametric upload: ") + hipGetErrorString(e);
        rc = -(int)e;
    } else {
        rc = parametric_on_device(ctx, batch, m, n, dA, db, dc, dbasis, nullptr, ddir, maximize, t_max, eps, mb,
                                  nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out, status_out);
    }
    (void)hipFree(buf);
    return rc;
}

// The argument checks shared by the three entry points (LP_OPTIMAL when they pass)
static int parametric_args(lp_context* ctx, const char* fn, double t_max, double eps, int max_breaks) {
    if (max_breaks < 0) LP_FAIL(ctx, LP_BAD_ARG, std::string(fn) + ": max_breaks must be >= 0");
    if (!(t_max >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(fn) + ": t_max must be >= 0");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(fn) + ": eps must be >= 0");
    return LP_OPTIMAL;
}

int lp_basis_parametric(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                        const int* basis, int maximize, const double* d, double t_max, double eps, int max_breaks,
                        int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                        int* leave_out, int* basis_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !d || !nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out ||
        !basis_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric: null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric: bad dimensions");
    if (max_breaks < 0) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric: max_breaks must be >= 0");
    parametric_none(0, m, max_breaks, basis, nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out);
    int rc = parametric_args(ctx, "lp_basis_parametric", t_max, eps, max_breaks);
    if (rc) return rc;
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    int status = LP_OPTIMAL;
    rc = parametric_upload(ctx, 1, A, m, n, b, c, basis, maximize, d, t_max, eps, max_breaks, nseg_out, t_out,
                           obj_out, slope_out, enter_out, leave_out, basis_out, &status);
    if (rc) return rc;
    if (status == LP_BAD_ARG) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric: the basis is not optimal at t = 0");
    return status;
}

int lp_basis_parametric_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                const double* c, const int* basis, int maximize, const double* d, double t_max,
                                double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out,
                                double* slope_out, int* enter_out, int* leave_out, int* basis_out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !d || !nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out ||
        !basis_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric_batched: null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric_batched: bad dimensions");
    const int rc = parametric_args(ctx, "lp_basis_parametric_batched", t_max, eps, max_breaks);
    if (rc) return rc;
    return parametric_upload(ctx, batch, A, m, n, b, c, basis, maximize, d, t_max, eps, max_breaks, nseg_out, t_out,
                             obj_out, slope_out, enter_out, leave_out, basis_out, status_out);
}

int lp_batched_parametric(lp_batched_problem* p, const double* d, double t_max, double eps, int max_breaks,
                          int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                          int* leave_out, int* basis_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!d || !nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out || !basis_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_parametric: null argument");
    int rc = parametric_args(ctx, "lp_batched_parametric", t_max, eps, max_breaks);
    if (rc) return rc;
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_parametric: the batch has not run");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const int m = p->m, n = p->n, mb = max_breaks;
    const size_t B = (size_t)p->batch;
    if (p->resident) {   // A, b, c, the final bases and the run statuses where the run left them; d goes up
        double* ddir = nullptr;
        LP_HIP(ctx, hipMalloc(&ddir, sizeof(double) * B * m));
        hipError_t e = hipMemcpyAsync(ddir, d, sizeof(double) * B * m, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(ddir);
            LP_HIP(ctx, e);
        }
        rc = parametric_on_device(ctx, p->batch, m, n, p->dA, p->db, p->dc, p->dbasis_out, p->dstatus, ddir,
                                  p->maximize, t_max, eps, mb, nseg_out, t_out, obj_out, slope_out, enter_out,
                                  leave_out, basis_out, status_out);
        (void)hipFree(ddir);
        return rc;
    }
    // per-LP fallback: the single-LP call on the kept inputs and each LP's final basis
    std::vector<int> basis((size_t)m);
    for (size_t k = 0; k < B; ++k) {
        if (p->two_phase || p->resolve) {
            std::memcpy(basis.data(), p->h_basis.data() + k * m, sizeof(int) * m);
        } else {
            rc = lp_simplex_download(p->lps[k], nullptr, basis.data(), nullptr, nullptr, nullptr, 0, nullptr);
            if (rc) return rc;
        }
        int st = p->status[k];
        parametric_none(k, m, mb, basis.data(), nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out);
        if (st == LP_OPTIMAL) {
            st = lp_basis_parametric(ctx, p->h_A.data() + k * m * n, m, n, p->h_b.data() + k * m,
                                     p->h_c.data() + k * n, basis.data(), p->maximize, d + k * m, t_max, eps, mb,
                                     nseg_out + k, t_out + k * (mb + 2), obj_out + k * (mb + 2),
                                     slope_out + k * (mb + 1), enter_out + k * (mb + 1), leave_out + k * (mb + 1),
                                     basis_out + k * m);
            if (st < 0) return st;
        }
        status_out[k] = st;
    }
    ctx->last_error.clear();
    return LP_OPTIMAL;
}

// ===========================================================================
// Parametric cost from an optimal basis (basis_parametric_cost.hip): one LP per workgroup for
// lp_basis_parametric_cost_fits(m, n), the single-LP launch path one LP after another beyond it
// ===========================================================================

int lp_basis_parametric_cost_fits(int m, int n) {
    return m > 0 && n >= m && lp_basis_parametric_cost_lds_bytes(m, n, nullptr) <= 160 * 1024 ? 1 : 0;
}

// Cost paths of `batch` LPs whose inputs (g included) are on the device; drun_status (device, or nullptr): LPs whose run
// status is not LP_OPTIMAL keep it and get nseg 0.  Outputs to the host.
static int parametric_cost_on_device(lp_context* ctx, int batch, int m, int n, const double* dA, const double* db,
                                     const double* dc, const int* dbasis, const int* drun_status, const double* dg,
                                     int maximize, double t_max, double eps, int mb, int* nseg_out, double* t_out,
                                     double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* basis_out,
                                     int* status_out) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch, nt = B * (mb + 2), ns = B * (mb + 1);
    const size_t bytes = sizeof(double) * (2 * nt + ns) + sizeof(int) * (2 * ns + B * m + 2 * B);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, bytes));
    BasisParametricCostDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    (void)lp_basis_parametric_cost_lds_bytes(m, n, &d.pitch);
    d.max_breaks = mb;
    d.eps = eps;
    d.t_max = t_max;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.g = dg;
    d.basis = dbasis;
    d.run_status = drun_status;
    d.t = reinterpret_cast<double*>(buf);
    d.obj = d.t + nt;
    d.slope = d.obj + nt;
    d.enter = reinterpret_cast<int*>(d.slope + ns);
    d.leave = d.enter + ns;
    d.basis_out = d.leave + ns;
    d.nseg = d.basis_out + B * m;
    d.status = d.nseg + B;
    std::vector<char> done(B, 1);   // the LP's outputs were written on the device
    std::vector<int> basis;         // per-LP path: the given bases
    int rc = LP_OPTIMAL;
    if (lp_basis_parametric_cost_fits(m, n)) {
        rc = lp_basis_parametric_cost_launch(ctx, d, maximize);
    } else {   // one LP after another: statuses and bases checked on the host
        std::vector<int> st(B, LP_OPTIMAL);
        basis.resize(B * m);
        hipError_t e = hipMemcpyAsync(basis.data(), dbasis, sizeof(int) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && drun_status)
            e = hipMemcpyAsync(st.data(), drun_status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(buf);
            LP_HIP(ctx, e);
        }
        for (size_t k = 0; k < B && rc >= 0; ++k) {
            done[k] = 0;
            if (st[k] != LP_OPTIMAL) continue;
            for (int t = 0; t < m; ++t)
                if (basis[k * m + t] < 0 || basis[k * m + t] >= n) st[k] = LP_BAD_ARG;
            if (st[k] != LP_OPTIMAL) continue;
            rc = lp_basis_parametric_cost_device(ctx, dA + k * m * n, m, n, db + k * m, dc + k * n, dbasis + k * m,
                                            dg + k * n, maximize, t_max, eps, mb, d.nseg + k, d.t + k * (mb + 2),
                                            d.obj + k * (mb + 2), d.slope + k * (mb + 1), d.enter + k * (mb + 1),
                                            d.leave + k * (mb + 1), d.basis_out + k * m);
            if (rc < 0) break;
            st[k] = rc;
            done[k] = rc == LP_OPTIMAL || rc == LP_UNBOUNDED || rc == LP_ITER_LIMIT;
        }
        if (rc >= 0) {
            rc = LP_OPTIMAL;
            e = hipMemcpyAsync(d.status, st.data(), sizeof(int) * B, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = -(int)e;
        }
    }
    if (rc == LP_OPTIMAL) {
        hipError_t e = hipMemcpyAsync(t_out, d.t, sizeof(double) * nt, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(obj_out, d.obj, sizeof(double) * nt, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(slope_out, d.slope, sizeof(double) * ns, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(enter_out, d.enter, sizeof(int) * ns, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(leave_out, d.leave, sizeof(int) * ns, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(basis_out, d.basis_out, sizeof(int) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nseg_out, d.nseg, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(status_out, d.status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ctx->last_error = std::string("basis parametric cost: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(buf);
    if (rc != LP_OPTIMAL) return rc;
    if (!basis.empty())   // the per-LP path writes the path only: the rest is NaN / -1, and LPs without one get it all
        for (size_t k = 0; k < B; ++k) {
            if (!done[k]) {
                parametric_none(k, m, mb, basis.data() + k * m, nseg_out, t_out, obj_out, slope_out, enter_out,
                                leave_out, basis_out);
                continue;
            }
            const int ns_k = nseg_out[k];
            for (int q = ns_k + 1; q < mb + 2; ++q) t_out[k * (mb + 2) + q] = obj_out[k * (mb + 2) + q] = NAN;
            for (int q = ns_k; q < mb + 1; ++q) {
                slope_out[k * (mb + 1) + q] = NAN;
                enter_out[k * (mb + 1) + q] = leave_out[k * (mb + 1) + q] = -1;
            }
        }
    return LP_OPTIMAL;
}

// Uploads `batch` LPs and their cost directions, then parametric_cost_on_device.
static int parametric_cost_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                  const double* c, const int* basis, int maximize, const double* g, double t_max,
                                  double eps, int mb, int* nseg_out, double* t_out, double* obj_out, double* slope_out,
                                  int* enter_out, int* leave_out, int* basis_out, int* status_out) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, dbl = B * ((size_t)m * n + m + 2 * n);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, sizeof(double) * dbl + sizeof(int) * B * m));
    double* dA = reinterpret_cast<double*>(buf);
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    double* dg = dc + B * n;
    int* dbasis = reinterpret_cast<int*>(dg + B * n);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dg, g, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    int rc = LP_OPTIMAL;
    if (e != hipSuccess) {
        ctx->last_error = std::string("basis parametric cost upload: ") + hipGetErrorString(e);
        rc = -(int)e;
    } else {
        rc = parametric_cost_on_device(ctx, batch, m, n, dA, db, dc, dbasis, nullptr, dg, maximize, t_max, eps, mb,
                                       nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out, status_out);
    }
    (void)hipFree(buf);
    return rc;
}

int lp_basis_parametric_cost(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                             const int* basis, int maximize, const double* g, double t_max, double eps, int max_breaks,
                             int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                             int* leave_out, int* basis_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !g || !nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out ||
        !basis_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric_cost: null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric_cost: bad dimensions");
    if (max_breaks < 0) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric_cost: max_breaks must be >= 0");
    parametric_none(0, m, max_breaks, basis, nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out);
    int rc = parametric_args(ctx, "lp_basis_parametric_cost", t_max, eps, max_breaks);
    if (rc) return rc;
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    int status = LP_OPTIMAL;
    rc = parametric_cost_upload(ctx, 1, A, m, n, b, c, basis, maximize, g, t_max, eps, max_breaks, nseg_out, t_out,
                                obj_out, slope_out, enter_out, leave_out, basis_out, &status);
    if (rc) return rc;
    if (status == LP_BAD_ARG) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric_cost: the basis is not optimal at t = 0");
    return status;
}

int lp_basis_parametric_cost_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                     const double* c, const int* basis, int maximize, const double* g, double t_max,
                                     double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out,
                                     double* slope_out, int* enter_out, int* leave_out, int* basis_out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !g || !nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out ||
        !basis_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric_cost_batched: null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_parametric_cost_batched: bad dimensions");
    const int rc = parametric_args(ctx, "lp_basis_parametric_cost_batched", t_max, eps, max_breaks);
    if (rc) return rc;
    return parametric_cost_upload(ctx, batch, A, m, n, b, c, basis, maximize, g, t_max, eps, max_breaks, nseg_out, t_out,
                                  obj_out, slope_out, enter_out, leave_out, basis_out, status_out);
}

int lp_batched_parametric_cost(lp_batched_problem* p, const double* g, double t_max, double eps, int max_breaks,
                               int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                               int* leave_out, int* basis_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!g || !nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out || !basis_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_parametric_cost: null argument");
    int rc = parametric_args(ctx, "lp_batched_parametric_cost", t_max, eps, max_breaks);
    if (rc) return rc;
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_parametric_cost: the batch has not run");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const int m = p->m, n = p->n, mb = max_breaks;
    const size_t B = (size_t)p->batch;
    if (p->resident) {   // A, b, c, the final bases and the run statuses where the run left them; g goes up
        double* dg = nullptr;
        LP_HIP(ctx, hipMalloc(&dg, sizeof(double) * B * n));
        hipError_t e = hipMemcpyAsync(dg, g, sizeof(double) * B * n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(dg);
            LP_HIP(ctx, e);
        }
        rc = parametric_cost_on_device(ctx, p->batch, m, n, p->dA, p->db, p->dc, p->dbasis_out, p->dstatus, dg,
                                       p->maximize, t_max, eps, mb, nseg_out, t_out, obj_out, slope_out, enter_out,
                                       leave_out, basis_out, status_out);
        (void)hipFree(dg);
        return rc;
    }
    // per-LP fallback: the single-LP call on the kept inputs and each LP's final basis
    std::vector<int> basis((size_t)m);
    for (size_t k = 0; k < B; ++k) {
        if (p->two_phase || p->resolve) {
            std::memcpy(basis.data(), p->h_basis.data() + k * m, sizeof(int) * m);
        } else {
            rc = lp_simplex_download(p->lps[k], nullptr, basis.data(), nullptr, nullptr, nullptr, 0, nullptr);
            if (rc) return rc;
        }
        int st = p->status[k];
        parametric_none(k, m, mb, basis.data(), nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out);
        if (st == LP_OPTIMAL) {
            st = lp_basis_parametric_cost(ctx, p->h_A.data() + k * m * n, m, n, p->h_b.data() + k * m,
                                          p->h_c.data() + k * n, basis.data(), p->maximize, g + k * n, t_max, eps, mb,
                                          nseg_out + k, t_out + k * (mb + 2), obj_out + k * (mb + 2),
                                          slope_out + k * (mb + 1), enter_out + k * (mb + 1), leave_out + k * (mb + 1),
                                          basis_out + k * m);
            if (st < 0) return st;
        }
        status_out[k] = st;
    }
    ctx->last_error.clear();
    return LP_OPTIMAL;
}

// ===========================================================================
// Depth-first branch-and-bound (batched_mip.hip): one integer LP per workgroup for lp_mip_fits shapes only; there is
// no per-LP host fallback
// ===========================================================================

int lp_mip_fits(int m, int n, int max_depth) { return lp_mip_fits_shape(m, n, max_depth) ? 1 : 0; }

// The search parameters and the mask (the basis and the problem arrays are checked by the callers).
static int mip_args(lp_context* ctx, const char* who, int m, int n, int n_orig, const int* integer, double int_tol,
                    double gap, int max_depth, int max_nodes) {
    if (!integer) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (max_depth < 0 || max_depth > LP_MIP_MAX_DEPTH)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": max_depth must be in [0, 64]");
    if (!(int_tol >= 0.0 && int_tol < 0.5)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": int_tol must be in [0, 0.5)");
    if (!(gap >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": gap must be >= 0");
    if (max_nodes < 1) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": max_nodes must be >= 1");
    for (int j = 0; j < n; ++j) {
        if (integer[j] != 0 && integer[j] != 1) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": mask entries must be 0 or 1");
        if (integer[j] && j >= n_orig)
            LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the mask marks a column beyond n_orig");
    }
    if (!lp_mip_fits_shape(m, n, max_depth))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the shape does not fit one CU's LDS (lp_mip_fits)");
    return LP_OPTIMAL;
}

// The search of `batch` problems whose A, b, c and root bases are on the device; drun_status (device, or nullptr):
// problems whose entry is not LP_OPTIMAL keep it.  The mask goes up; outputs to the host.
static int mip_on_device(lp_context* ctx, int batch, int m, int n, int n_orig, const double* dA, const double* db,
                         const double* dc, const int* dbasis, const int* drun_status, const int* integer, int maximize,
                         double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter,
                         double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out,
                         int* status_out) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch;
    const size_t bytes = sizeof(double) * (B * n_orig + 2 * B) + sizeof(int) * (B * 6 + n);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, bytes));
    BatchedMipDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.n_orig = n_orig;
    d.maximize = maximize ? 1 : 0;
    d.max_iter = max_iter;
    d.max_depth = max_depth;
    d.max_nodes = max_nodes;
    d.eps = eps;
    d.int_tol = int_tol;
    d.gap = gap;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.basis_in = dbasis;
    d.run_status = drun_status;
    d.x = reinterpret_cast<double*>(buf);
    d.obj = d.x + B * n_orig;
    d.bound = d.obj + B;
    d.found = reinterpret_cast<int*>(d.bound + B);
    d.stats = d.found + B;
    d.status = d.stats + B * 4;
    int* dmask = d.status + B;
    d.integer = dmask;
    hipError_t e = hipMemcpyAsync(dmask, integer, sizeof(int) * n, hipMemcpyHostToDevice, s);
    int rc = e == hipSuccess ? lp_batched_mip_launch(ctx, d) : -(int)e;
    if (rc == LP_OPTIMAL) {
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(x_out, d.x, sizeof(double) * B * n_orig, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(obj_out, d.obj, sizeof(double) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(bound_out, d.bound, sizeof(double) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(found_out, d.found, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(stats_out, d.stats, sizeof(int) * B * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(status_out, d.status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ctx->last_error = std::string("batched MIP: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    } else if (rc < 0) {
        ctx->last_error = std::string("batched MIP upload: ") + hipGetErrorString(e);
    }
    (void)hipFree(buf);
    return rc;
}

// Uploads `batch` problems and their root bases, then mip_on_device.
static int mip_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                      const int* basis, int maximize, int n_orig, const int* run_status, const int* integer,
                      double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter,
                      double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out,
                      int* status_out) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, dbl = B * ((size_t)m * n + m + n);
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, sizeof(double) * dbl + sizeof(int) * B * (m + 1)));
    double* dA = reinterpret_cast<double*>(buf);
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    int* dbasis = reinterpret_cast<int*>(dc + B * n);
    int* drun = dbasis + B * m;
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && run_status) e = hipMemcpyAsync(drun, run_status, sizeof(int) * B, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    int rc = LP_OPTIMAL;
    if (e != hipSuccess) {
        ctx->last_error = std::string("batched MIP upload: ") + hipGetErrorString(e);
        rc = -(int)e;
    } else {
        rc = mip_on_device(ctx, batch, m, n, n_orig, dA, db, dc, dbasis, run_status ? drun : nullptr, integer,
                           maximize, eps, int_tol, gap, max_depth, max_nodes, max_iter, x_out, obj_out, bound_out,
                           found_out, stats_out, status_out);
    }
    (void)hipFree(buf);
    return rc;
}

int lp_mip_solve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const int* basis,
                 int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth,
                 int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out,
                 int* stats_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_solve: null argument");
    int rc = check_canonical(ctx, A, m, n, b, c, basis, n_orig);
    if (rc) return rc;
    rc = mip_args(ctx, "lp_mip_solve", m, n, n_orig, integer, int_tol, gap, max_depth, max_nodes);
    if (rc) return rc;
    int status = LP_OPTIMAL;
    rc = mip_upload(ctx, 1, A, m, n, b, c, basis, maximize, n_orig, nullptr, integer, eps, int_tol, gap, max_depth,
                    max_nodes, max_iter, x_out, obj_out, bound_out, found_out, stats_out, &status);
    if (rc) return rc;
    if (status == LP_BAD_ARG) LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_solve: the basis is neither primal nor dual feasible");
    return status;
}

int lp_mip_solve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                         const int* basis, int maximize, int n_orig, const int* integer, double eps, double int_tol,
                         double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out,
                         double* bound_out, int* found_out, int* stats_out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_solve_batched: null argument");
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    for (int k = 0; k < batch; ++k) {
        int rc = check_canonical(ctx, A ? A + (size_t)k * m * n : nullptr, m, n, b ? b + (size_t)k * m : nullptr,
                                 c ? c + (size_t)k * n : nullptr, basis ? basis + (size_t)k * m : nullptr, n_orig);
        if (rc) return rc;
    }
    const int rc = mip_args(ctx, "lp_mip_solve_batched", m, n, n_orig, integer, int_tol, gap, max_depth, max_nodes);
    if (rc) return rc;
    return mip_upload(ctx, batch, A, m, n, b, c, basis, maximize, n_orig, nullptr, integer, eps, int_tol, gap,
                      max_depth, max_nodes, max_iter, x_out, obj_out, bound_out, found_out, stats_out, status_out);
}

int lp_batched_mip(lp_batched_problem* p, const int* integer, double eps, double int_tol, double gap, int max_depth,
                   int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out,
                   int* stats_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_mip: null argument");
    int rc = mip_args(ctx, "lp_batched_mip", p->m, p->n, p->n_orig, integer, int_tol, gap, max_depth, max_nodes);
    if (rc) return rc;
    if (p->pivot_rule != LP_PIVOT_DANTZIG) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_mip: Dantzig's rule only");
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_mip: the batch has not run");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const int m = p->m, n = p->n;
    const size_t B = (size_t)p->batch;
    if (p->resident)   // A, b, c, the final bases and the run statuses where the run left them
        return mip_on_device(ctx, p->batch, m, n, p->n_orig, p->dA, p->db, p->dc, p->dbasis_out, p->dstatus, integer,
                             p->maximize, eps, int_tol, gap, max_depth, max_nodes, max_iter, x_out, obj_out,
                             bound_out, found_out, stats_out, status_out);
    // per-LP runs: the kept inputs and each LP's final basis go up, then the same kernel
    std::vector<int> basis(B * m);
    for (size_t k = 0; k < B; ++k) {
        if (p->two_phase || p->resolve) {
            std::memcpy(basis.data() + k * m, p->h_basis.data() + k * m, sizeof(int) * m);
        } else {
            rc = lp_simplex_download(p->lps[k], nullptr, basis.data() + k * m, nullptr, nullptr, nullptr, 0, nullptr);
            if (rc) return rc;
        }
    }
    return mip_upload(ctx, p->batch, p->h_A.data(), m, n, p->h_b.data(), p->h_c.data(), basis.data(), p->maximize,
                      p->n_orig, p->status.data(), integer, eps, int_tol, gap, max_depth, max_nodes, max_iter, x_out,
                      obj_out, bound_out, found_out, stats_out, status_out);
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
    char* buf = nullptr;
    LP_HIP(ctx, hipMalloc(&buf, sizeof(double) * dbl + sizeof(int) * ints));
    BatchedBoundedDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    (void)lp_bounded_lds_bytes(m, n, &d.pitch);
    d.maximize = maximize ? 1 : 0;
    d.max_iter = max_iter;
    d.eps = eps;
    double* dA = reinterpret_cast<double*>(buf);
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
    int rc = e == hipSuccess ? lp_batched_bounded_launch(ctx, d) : -(int)e;
    if (rc == LP_OPTIMAL) {
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(x.data(), d.x, sizeof(double) * B * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(basis_out, d.basis_out, sizeof(int) * B * m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(at_upper_out, d.at_upper, sizeof(int) * B * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(iters_out, d.iters, sizeof(int) * B * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(status_out, d.status, sizeof(int) * B, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ctx->last_error = std::string("batched bounded simplex: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    } else if (rc < 0) {
        ctx->last_error = std::string("batched bounded simplex upload: ") + hipGetErrorString(e);
    }
    (void)hipFree(buf);
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
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    const int rc = bounded_args(ctx, "lp_simplex_bounded_batched", batch, A, m, n, b, c, lo, hi, n_orig);
    if (rc) return rc;
    return bounded_solve(ctx, batch, A, m, n, b, c, lo, hi, maximize, n_orig, eps, max_iter, x_out, basis_out,
                         at_upper_out, obj_out, iters_out, status_out);
}

}  // extern "C"
