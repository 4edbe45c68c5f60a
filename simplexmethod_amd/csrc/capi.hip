// capi.hip — the extern "C" boundary (include/simplexmethod_amd.h): argument checks that
// mirror the reference's constructors, uploads/downloads, and dispatch to the kernels.
#include <chrono>
#include <cmath>
#include <cstdio>

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
// simplex
// ===========================================================================

// Canonical's constructor checks (Canonical.cpp:27-46) + SetOriginalVariablesCount (:156-163).
static int check_canonical(lp_context* ctx, const double* A, int m, int n, const double* b,
                           const double* c, const int* basis, int n_orig) {
    if (!A || !b || !c || !basis) LP_FAIL(ctx, LP_BAD_ARG, "null problem array");
    if (m <= 0 || n <= 0) LP_FAIL(ctx, LP_BAD_ARG, "empty problem");
    if (n < m) LP_FAIL(ctx, LP_BAD_ARG, "fewer columns than rows");
    if (n_orig <= 0 || n_orig > n) LP_FAIL(ctx, LP_BAD_ARG, "bad original variable count");
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    return LP_OPTIMAL;
}

void lp_simplex_free(lp_simplex_problem* p) {
    if (!p) return;
    lp_context* ctx = p->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);   // the arena goes back to the pool: nothing may still use it
    lp_pool_release(ctx, p->arena, p->arena_bytes);
    (void)hipFree(p->dscratchT);
    (void)hipFree(p->ov_T);
    (void)hipFree(p->ov_vec);
    (void)hipFree(p->look.stamps);
    if (p->h_state) {   // pinned block + events: kept for the next problem of this context
        lp_context::HostBundle hb;
        hb.pinned = p->h_state;
        hb.ev[0] = p->ev0; hb.ev[1] = p->ev1; hb.ev[2] = p->res_ev0; hb.ev[3] = p->res_ev1;
        if (ctx->bundles.size() < 8) {
            ctx->bundles.push_back(hb);
        } else {
            (void)hipHostFree(hb.pinned);
            for (hipEvent_t e : hb.ev)
                if (e) (void)hipEventDestroy(e);
        }
    }
    for (hipEvent_t e : p->upd_events) (void)hipEventDestroy(e);
    delete p;
}

namespace {
// T (rows x ld, row-major) <- [A | b] with the cost row c underneath, from the column-major A the
// caller holds (Eigen's layout): a tiled transpose on the device instead of a strided host loop.
__global__ __launch_bounds__(256) void k_build_tableau(const double* __restrict__ Acol, const double* __restrict__ b,
                                                       const double* __restrict__ c, double* __restrict__ T,
                                                       int m, int n, int ld) {
    __shared__ double tile[32][33];
    const int j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int q = ty; q < 32; q += 8) {   // read: consecutive threads along i (contiguous in column-major A)
        const int j = j0 + q, i = i0 + tx;
        tile[q][tx] = (j < n && i < m) ? Acol[(size_t)j * m + i] : 0.0;
    }
    __syncthreads();
    for (int q = ty; q < 32; q += 8) {   // write: consecutive threads along j (contiguous in row-major T)
        const int i = i0 + q, j = j0 + tx;
        if (i < m && j < n) T[(size_t)i * ld + j] = tile[tx][q];
    }
    if (blockIdx.x == 0) {   // column n (b), padding, and (first row of blocks) the cost row
        for (int q = threadIdx.x; q < 32; q += 256) {
            const int i = i0 + q;
            if (i < m) {
                T[(size_t)i * ld + n] = b[i];
                for (int j = n + 1; j < ld; ++j) T[(size_t)i * ld + j] = 0.0;
            }
        }
    }
    if (blockIdx.y == 0) {
        for (int q = threadIdx.x; q < 32; q += 256) {
            const int j = j0 + q;
            if (j < n) T[(size_t)m * ld + j] = c[j];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (int j = n; j < ld; ++j) T[(size_t)m * ld + j] = 0.0;
    }
}
}  // namespace

int lp_simplex_upload(lp_context* ctx, const double* A, int m, int n, const double* b,
                      const double* c, const int* basis_in, int maximize, int n_orig,
                      lp_simplex_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    int rc = check_canonical(ctx, A, m, n, b, c, basis_in, n_orig);
    if (rc) return rc;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    lp_simplex_problem* p = new lp_simplex_problem();
    p->ctx = ctx;
    p->n_orig = n_orig;
    p->h_c.assign(c, c + n);
    SimplexDev& d = p->dev;
    d.m = m;
    d.n = n;
    d.ld = ((n + 1 + 7) / 8) * 8;
    d.maximize = maximize ? 1 : 0;
    d.trace_cap = 16384;
    const size_t rows = (size_t)m + 1;
    p->tableau_bytes = sizeof(double) * rows * (size_t)d.ld;
#define LP_TRY(expr)                        \
    do {                                    \
        hipError_t _e = (expr);             \
        if (_e != hipSuccess) {             \
            ctx->last_error = #expr;        \
            lp_simplex_free(p);             \
            return -(int)_e;                \
        }                                   \
    } while (0)
    // ---- one arena for everything on the device (taken from / returned to the context's pool:
    // a repeated one-shot solve of the same shape allocates nothing)
    LookDev& la = p->look;
    la.J = lp_lookahead_pick_j(m, n);
    la.rows_pad = ((m + 1 + 7) / 8) * 8;
    const size_t J = (size_t)(la.J > 0 ? la.J : 1);
    const bool resident = lp_resident_plan(m, n, &p->res) != 0;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t staging_bytes = std::max(p->tableau_bytes, sizeof(double) * ((size_t)m * n + m + n) + 256);
    const size_t oT = take(p->tableau_bytes), oT0 = take(staging_bytes);
    const size_t olcol = take(sizeof(double) * rows), oprow = take(sizeof(double) * (size_t)d.ld);
    const size_t obasis = take(sizeof(int) * (size_t)m), obasis0 = take(sizeof(int) * (size_t)m);
    const size_t onb = take((size_t)n), onb0 = take((size_t)n), oused = take((size_t)m);
    const size_t orowpos = take(sizeof(int) * (size_t)m);
    const size_t otre = take(sizeof(int) * (size_t)d.trace_cap), otrl = take(sizeof(int) * (size_t)d.trace_cap);
    const size_t ostate = take(sizeof(SimplexState)), odx = take(sizeof(double) * (size_t)n);
    const size_t oetaL = take(sizeof(double) * J * (size_t)la.rows_pad), oetaP = take(sizeof(double) * J * (size_t)d.ld);
    const size_t odvec = take(sizeof(double) * (size_t)d.ld), orhs = take(sizeof(double) * (size_t)la.rows_pad);
    const size_t opiv = take(sizeof(int) * 2 * J), ocount = take(sizeof(int));
    const size_t ocomm = resident ? take(p->res.comm_bytes) : 0;
    {
        size_t got = 0;
        LP_TRY(lp_pool_alloc(ctx, &p->arena, off, &got));
        p->arena_bytes = got;
    }
    char* base = static_cast<char*>(p->arena);
    d.T = reinterpret_cast<double*>(base + oT);
    p->dT0 = reinterpret_cast<double*>(base + oT0);
    d.lcol = reinterpret_cast<double*>(base + olcol);
    d.prow = reinterpret_cast<double*>(base + oprow);
    d.basis = reinterpret_cast<int*>(base + obasis);
    p->dbasis0 = reinterpret_cast<int*>(base + obasis0);
    d.nonbasic = reinterpret_cast<unsigned char*>(base + onb);
    p->dnonbasic0 = reinterpret_cast<unsigned char*>(base + onb0);
    d.rowused = reinterpret_cast<unsigned char*>(base + oused);
    d.rowpos = reinterpret_cast<int*>(base + orowpos);
    d.trace_enter = reinterpret_cast<int*>(base + otre);
    d.trace_leave = reinterpret_cast<int*>(base + otrl);
    d.state = reinterpret_cast<SimplexState*>(base + ostate);
    p->dx = reinterpret_cast<double*>(base + odx);
    la.etaL = reinterpret_cast<double*>(base + oetaL);
    la.etaP = reinterpret_cast<double*>(base + oetaP);
    la.dvec = reinterpret_cast<double*>(base + odvec);
    la.rhs = reinterpret_cast<double*>(base + orhs);
    la.piv = reinterpret_cast<int*>(base + opiv);
    la.count = reinterpret_cast<int*>(base + ocount);
    if (resident) p->res.comm = base + ocomm;
    if (!ctx->bundles.empty()) {
        const lp_context::HostBundle hb = ctx->bundles.back();
        ctx->bundles.pop_back();
        p->h_state = static_cast<SimplexState*>(hb.pinned);
        p->ev0 = hb.ev[0]; p->ev1 = hb.ev[1]; p->res_ev0 = hb.ev[2]; p->res_ev1 = hb.ev[3];
    } else {
        LP_TRY(hipHostMalloc(&p->h_state, sizeof(SimplexState) + 64));
        LP_TRY(hipEventCreate(&p->ev0));
        LP_TRY(hipEventCreate(&p->ev1));
    }
    hipStream_t s = ctx->stream;
    LP_TRY(hipMemsetAsync(la.count, 0, sizeof(int), s));

    // ---- initial tableau [A | b] with the cost row c underneath, row-major: A goes up as the caller
    // holds it (column-major) into the staging area and is transposed on the device
    double* dA = p->dT0;
    double* db = dA + (size_t)m * n;
    double* dc = db + m;
    std::vector<unsigned char> nonbasic((size_t)n, 1);
    for (int t = 0; t < m; ++t) nonbasic[(size_t)basis_in[t]] = 0;
    LP_TRY(hipMemcpyAsync(dA, A, sizeof(double) * (size_t)m * n, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(db, b, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(dc, c, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_build_tableau, dim3(lp_ceil_div(n, 32), lp_ceil_div(m, 32)), 256, 0, s, dA, db, dc, d.T, m, n,
                       d.ld);
    LP_TRY(hipMemcpyAsync(d.basis, basis_in, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->dbasis0, basis_in, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(d.nonbasic, nonbasic.data(), (size_t)n, hipMemcpyHostToDevice, s));
    LP_TRY(hipMemcpyAsync(p->dnonbasic0, nonbasic.data(), (size_t)n, hipMemcpyHostToDevice, s));
    LP_TRY(hipStreamSynchronize(s));
    LP_TRY(hipGetLastError());
#undef LP_TRY

    // computeBFS (SimplexSolover.h:423): nothing to do for the slack identity basis with
    // zero basic costs (Symmetrical::ToCanonical, Symmetrical.cpp:169-188); otherwise m
    // Gauss-Jordan pivots on the device.
    bool identity = true, zero_costs = true;
    for (int t = 0; t < m && identity; ++t) {
        if (c[basis_in[t]] != 0.0) zero_costs = false;
        for (int i = 0; i < m && identity; ++i)
            if (A[(size_t)basis_in[t] * m + i] != ((i == t) ? 1.0 : 0.0)) identity = false;
    }
    p->init_status = LP_OPTIMAL;
    if (identity && !zero_costs) {
        // unit-vector basis with costs (the artificial basis of a phase-I problem): the crash pivots
        // only touch the reduced-cost row — one pass instead of m rank-1 updates
        rc = lp_simplex_price_out_identity(p);
        if (rc) {
            lp_simplex_free(p);
            return rc;
        }
    } else if (!identity) {
        rc = lp_simplex_crash(p);
        if (rc < 0) {
            lp_simplex_free(p);
            return rc;
        }
        p->init_status = rc;
    }
    hipError_t e = hipMemcpyAsync(p->dT0, d.T, p->tableau_bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        lp_simplex_free(p);
        return -(int)e;
    }
    *problem_out = p;
    return LP_OPTIMAL;
}

int lp_simplex_reset(lp_simplex_problem* p) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const SimplexDev& d = p->dev;
    hipStream_t s = ctx->stream;
    LP_HIP(ctx, hipMemcpyAsync(d.T, p->dT0, p->tableau_bytes, hipMemcpyDeviceToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(d.basis, p->dbasis0, sizeof(int) * (size_t)d.m, hipMemcpyDeviceToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(d.nonbasic, p->dnonbasic0, (size_t)d.n, hipMemcpyDeviceToDevice, s));
    LP_HIP(ctx, hipStreamSynchronize(s));
    p->last_status = -100;
    p->last_iters = 0;
    return LP_OPTIMAL;
}

int lp_simplex_run(lp_simplex_problem* p, double eps, int max_iter, int algo,
                   lp_simplex_stats* stats_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
    if (p->init_status != LP_OPTIMAL) {  // "Singular basis matrix", SimplexSolover.h:125-126
        if (stats_out) stats_out->status = p->init_status;
        p->last_status = p->init_status;
        return p->init_status;
    }
    const bool asked_auto = algo == LP_SIMPLEX_ALGO_AUTO;
    if (algo == LP_SIMPLEX_ALGO_AUTO)
        algo = p->res.G >= 1 ? LP_SIMPLEX_ALGO_RESIDENT
               : p->look.J >= 3 ? LP_SIMPLEX_ALGO_LOOKAHEAD   // (depth 2, 1536 x 3072: 20.0 us per pivot against the overlapped path's 18.4)
               : lp_overlap_auto(p->dev.m) ? LP_SIMPLEX_ALGO_OVERLAP : LP_SIMPLEX_ALGO_LAUNCH;
    if (algo == LP_SIMPLEX_ALGO_OVERLAP && asked_auto && lp_overlap_prepare(p) != LP_OPTIMAL) {
        (void)hipGetLastError();   // no memory for the second tableau buffer: the launch pair per pivot
        ctx->last_error.clear();
        algo = LP_SIMPLEX_ALGO_LAUNCH;
    }
    const int asked = algo;
    p->last_algo = algo;   // (every path overwrites it with the algorithm that answered; an early error return reports the one asked for)
    int rc;
    switch (algo) {
        case LP_SIMPLEX_ALGO_RESIDENT:
            if (p->res.G < 1)
                LP_FAIL(ctx, LP_BAD_ARG, "chip-resident simplex needs m <= 960 and ceil(n / columns per workgroup) <= 256 workgroups");
            rc = lp_simplex_run_resident(p, eps, max_iter, stats_out);
            break;
        case LP_SIMPLEX_ALGO_LAUNCH:
            rc = lp_simplex_run_launch(p, eps, max_iter, stats_out);
            break;
        case LP_SIMPLEX_ALGO_OVERLAP:
            rc = lp_simplex_run_overlap(p, eps, max_iter, stats_out);
            break;
        case LP_SIMPLEX_ALGO_LOOKAHEAD: {
            if (p->look.J < 1)
                LP_FAIL(ctx, LP_BAD_ARG, "look-ahead selector does not fit LDS for this m, n");
            rc = lp_lookahead_prepare(p);
            if (rc) return rc;
            rc = lp_simplex_run_lookahead(p, eps, max_iter, stats_out);
            break;
        }
        default:
            LP_FAIL(ctx, LP_BAD_ARG, "unknown simplex algorithm id");
    }
    if (stats_out) {   // which algorithm produced the answer (a chip-resident hand-off that timed out is re-run)
        stats_out->algo_used = p->last_algo;
        stats_out->fell_back = (asked == LP_SIMPLEX_ALGO_RESIDENT && p->last_algo != LP_SIMPLEX_ALGO_RESIDENT) ? 1 : 0;
    }
    return rc;
}

int lp_simplex_profile(lp_simplex_problem* p, int on) {
    if (!p) return LP_BAD_ARG;
    p->profile_updates = on != 0;
    return LP_OPTIMAL;
}

int lp_simplex_download(lp_simplex_problem* p, double* x_out, int* basis_out, double* obj_out,
                        int* trace_enter, int* trace_leave, int trace_cap, double* tableau_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const SimplexDev& d = p->dev;
    hipStream_t s = ctx->stream;
    std::vector<double> x((size_t)d.n, 0.0);
    if (x_out || obj_out) {
        lp_simplex_extract_x(p, p->dx);
        LP_HIP(ctx, hipMemcpyAsync(x.data(), p->dx, sizeof(double) * (size_t)d.n, hipMemcpyDeviceToHost, s));
    }
    if (basis_out)
        LP_HIP(ctx, hipMemcpyAsync(basis_out, d.basis, sizeof(int) * (size_t)d.m, hipMemcpyDeviceToHost, s));
    const int k = std::min(trace_cap, std::min(p->last_iters, d.trace_cap));
    if (trace_enter && k > 0)
        LP_HIP(ctx, hipMemcpyAsync(trace_enter, d.trace_enter, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, s));
    if (trace_leave && k > 0)
        LP_HIP(ctx, hipMemcpyAsync(trace_leave, d.trace_leave, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, s));
    std::vector<double> T;
    if (tableau_out) {
        T.resize(((size_t)d.m + 1) * (size_t)d.ld);
        LP_HIP(ctx, hipMemcpyAsync(T.data(), d.T, p->tableau_bytes, hipMemcpyDeviceToHost, s));
    }
    LP_HIP(ctx, hipStreamSynchronize(s));
    LP_HIP(ctx, hipGetLastError());
    if (x_out)  // x.head(n_orig), SimplexSolover.h:435-438
        for (int j = 0; j < p->n_orig; ++j) x_out[j] = x[(size_t)j];
    if (obj_out) {  // Canonical::Evaluate, Canonical.cpp:86
        double z = 0.0;
        for (int j = 0; j < d.n; ++j) z += p->h_c[(size_t)j] * x[(size_t)j];
        *obj_out = z;
    }
    if (tableau_out)
        for (int i = 0; i <= d.m; ++i)
            std::memcpy(tableau_out + (size_t)i * (d.n + 1), T.data() + (size_t)i * d.ld,
                        sizeof(double) * (size_t)(d.n + 1));
    return LP_OPTIMAL;
}

int lp_simplex_solve(lp_context* ctx, const double* A, int m, int n, const double* b,
                     const double* c, const int* basis_in, int maximize, int n_orig, double eps,
                     int max_iter, double* x_out, int* basis_out, double* obj_out, int* iters_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out) LP_FAIL(ctx, LP_BAD_ARG, "x_out is null");
    lp_simplex_problem* p = nullptr;
    int rc = lp_simplex_upload(ctx, A, m, n, b, c, basis_in, maximize, n_orig, &p);
    if (rc) return rc;
    lp_simplex_stats st;
    rc = lp_simplex_run(p, eps, max_iter, LP_SIMPLEX_ALGO_AUTO, &st);
    if (iters_out) *iters_out = st.pivots;
    if (rc == LP_OPTIMAL) {
        rc = lp_simplex_download(p, x_out, basis_out, obj_out, nullptr, nullptr, 0, nullptr);
    } else if (rc > 0 && basis_out) {
        (void)lp_simplex_download(p, nullptr, basis_out, nullptr, nullptr, nullptr, 0, nullptr);
    }
    lp_simplex_free(p);
    return rc;
}

int lp_simplex_row(lp_simplex_problem* p, int row, double* out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!out || row < 0 || row > p->dev.m) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_row: bad row or null output");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    LP_HIP(ctx, hipMemcpyAsync(out, p->dev.T + (size_t)row * p->dev.ld, sizeof(double) * (size_t)(p->dev.n + 1),
                               hipMemcpyDeviceToHost, ctx->stream));
    LP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LP_OPTIMAL;
}

int lp_simplex_force_pivot(lp_simplex_problem* p, int row, int col) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (row < 0 || row >= p->dev.m || col < 0 || col >= p->dev.n)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_force_pivot: position outside the tableau");
    if (p->init_status != LP_OPTIMAL) LP_FAIL(ctx, LP_SINGULAR, "lp_simplex_force_pivot: the initial basis was singular");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    return lp_simplex_force(p, row, col);
}

// Two-phase simplex: the host logic of the flow, every pivot on the GPU.
int lp_simplex_two_phase(lp_context* ctx, const double* A, int m, int n, const double* b,
                         const double* c, int maximize, int n_orig, double eps, int max_iter,
                         double* x_out, int* basis_out, double* obj_out, int* iters_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !x_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_two_phase: null argument");
    if (m <= 0 || n < m || n_orig <= 0 || n_orig > n) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_two_phase: bad dimensions");
    const int na = n + m;
    std::vector<double> A1((size_t)m * na, 0.0), b1((size_t)m), c1((size_t)na, 0.0), xa((size_t)na);
    std::vector<int> N((size_t)m);
    int it[3] = {0, 0, 0};
    if (iters_out) std::memcpy(iters_out, it, sizeof(it));
    // -DLP_TWO_PHASE_TRACE (diagnostic builds, scripts/two_phase_trace.py): wall time of each stage on stderr
#ifdef LP_TWO_PHASE_TRACE
    const bool trace = true;
#else
    const bool trace = false;
#endif
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t_prev = now();
    auto stage = [&](const char* name) {
        if (!trace) return;
        const auto t = now();
        fprintf(stderr, "[two_phase] %-28s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    };
    // make_b_nonneg (:61-68) and createAuxiliaryProblem (:70-95)
    std::vector<char> flip((size_t)m);
    for (int i = 0; i < m; ++i) {
        flip[i] = b[i] < -eps;
        b1[i] = flip[i] ? -b[i] : b[i];
        A1[(size_t)(n + i) * m + i] = 1.0;
    }
    for (int j = 0; j < n; ++j) {   // (column by column: both matrices are column-major)
        const double* src = A + (size_t)j * m;
        double* dst = A1.data() + (size_t)j * m;
        for (int i = 0; i < m; ++i) dst[i] = flip[i] ? -src[i] : src[i];
    }
    for (int j = n; j < na; ++j) c1[j] = 1.0;
    for (int t = 0; t < m; ++t) N[t] = n + t;
    stage("auxiliary problem (host)");
    // ---- phase I: minimise the sum of the artificials
    lp_simplex_problem* p = nullptr;
    int rc = lp_simplex_upload(ctx, A1.data(), m, na, b1.data(), c1.data(), N.data(), 0, na, &p);
    if (rc) return rc;
    stage("upload");
    lp_simplex_stats st;
    rc = lp_simplex_run(p, eps, max_iter, LP_SIMPLEX_ALGO_AUTO, &st);
    it[0] = st.pivots;
    stage("phase I run");
    if (rc == LP_OPTIMAL) rc = lp_simplex_download(p, xa.data(), N.data(), nullptr, nullptr, nullptr, 0, nullptr);
    stage("phase I download");
    if (rc == LP_OPTIMAL) {
        double sum = 0.0;  // :347-350
        for (int i = 0; i < m; ++i) sum += xa[(size_t)n + i];
        if (sum > eps) {  // :352-353
            rc = LP_INFEASIBLE;
            ctx->last_error = "two-phase: the problem has no feasible solution (phase I optimum > eps)";
        }
    }
    if (rc == LP_OPTIMAL) {
        // replaceArtificialColumns (:331-381): every artificial still basic (at level 0) leaves for
        // the first non-basic original column with |T[pos][cand]| > eps, chosen on the device; the
        // positions are known from the phase-I basis, so all pivots are queued behind one another
        std::vector<int> positions;
        for (int pos = 0; pos < m; ++pos)
            if (N[pos] >= n) positions.push_back(pos);
        if (!positions.empty()) {
            rc = lp_simplex_driveout(p, positions.data(), (int)positions.size(), n, eps, &it[1]);
            if (rc == LP_SINGULAR)   // :372-380: linearly dependent constraints
                ctx->last_error = "two-phase: an artificial variable cannot leave the basis (linearly dependent constraints)";
        }
    }
    // ---- phase II (:383-404) continues on the phase-I tableau: original costs priced out over the
    // current basis, artificial columns barred — no re-inversion of the basis from [A' | b']
    stage("drive-out");
    if (rc == LP_OPTIMAL) rc = lp_simplex_phase2_costs(p, c, n, maximize, n_orig);
    stage("phase II costs");
    if (rc == LP_OPTIMAL) {
        rc = lp_simplex_run(p, eps, max_iter, LP_SIMPLEX_ALGO_AUTO, &st);
        it[2] = st.pivots;
        stage("phase II run");
        if (rc == LP_OPTIMAL)
            rc = lp_simplex_download(p, x_out, N.data(), obj_out, nullptr, nullptr, 0, nullptr);
        else if (rc > 0)
            (void)lp_simplex_download(p, nullptr, N.data(), nullptr, nullptr, nullptr, 0, nullptr);
    } else if (rc == LP_SINGULAR || rc == LP_INFEASIBLE) {
        (void)lp_simplex_download(p, nullptr, N.data(), nullptr, nullptr, nullptr, 0, nullptr);
    }
    stage("phase II download");
    lp_simplex_free(p);
    stage("free");
    if (basis_out) std::memcpy(basis_out, N.data(), sizeof(int) * (size_t)m);
    if (iters_out) std::memcpy(iters_out, it, sizeof(it));
    return rc;
}

// Diagnostic: switches the look-ahead selector's per-phase cycle stamps on (cap_pivots > 0)
// and, after a run, copies them out: 8 stamps per pivot (s_memtime ticks).
int lp_debug_simplex_stamps(lp_simplex_problem* p, int cap_pivots, unsigned long long* out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (!p->look.stamps) {
        if (cap_pivots <= 0) return LP_OPTIMAL;
        const size_t bytes = sizeof(unsigned long long) * 8 * (size_t)(cap_pivots + 64);
        LP_HIP(ctx, hipMalloc(&p->look.stamps, bytes));
        LP_HIP(ctx, hipMemset(p->look.stamps, 0, bytes));
        return LP_OPTIMAL;
    }
    if (out)
        LP_HIP(ctx, hipMemcpy(out, p->look.stamps, sizeof(unsigned long long) * 8 * (size_t)cap_pivots, hipMemcpyDeviceToHost));
    return LP_OPTIMAL;
}

int lp_bench_rank1_update(lp_simplex_problem* p, int row, int col, int iters,
                          float* ms_per_launch_out) {
    if (!p) return LP_BAD_ARG;
    LP_HIP(p->ctx, hipSetDevice(p->ctx->device));
    return lp_simplex_bench_update(p, row, col, iters, ms_per_launch_out);
}

int lp_bench_rankj_update(lp_simplex_problem* p, int iters, float* ms_per_launch_out,
                          int* pivots_per_launch_out) {
    if (!p) return LP_BAD_ARG;
    LP_HIP(p->ctx, hipSetDevice(p->ctx->device));
    return lp_lookahead_bench_update(p, iters, ms_per_launch_out, pivots_per_launch_out);
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
        const double* Ak = A + (size_t)k * m * n;
        const double* ck = c + (size_t)k * n;
        const int* bk = basis_in + (size_t)k * m;
        for (int t = 0; t < m && identity; ++t) {
            if (ck[bk[t]] != 0.0) identity = false;
            for (int i = 0; i < m && identity; ++i)
                if (Ak[(size_t)bk[t] * m + i] != ((i == t) ? 1.0 : 0.0)) identity = false;
        }
    }
    int pitch = 0;
    const size_t lds = lp_batched_lds_bytes(m, n, &pitch);
    p->resident = identity && lds <= 160 * 1024;
    if (!p->resident) {
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

int lp_batched_run(lp_batched_problem* p, double eps, int max_iter, float* ms_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (p->resident) {
        p->dev.eps = eps;
        p->dev.max_iter = max_iter;
        if (const char* sv = getenv("LP_BATCHED_STAMPS"); sv && !p->dev.stamps) {   // diagnostic build of the kernel (scripts/stamp_batched.py)
            LP_HIP(ctx, hipMalloc(&p->dev.stamps, sizeof(unsigned long long) * 64));   // 32 phase sums + 2 per wave (16 waves)
            LP_HIP(ctx, hipMemset(p->dev.stamps, 0, sizeof(unsigned long long) * 64));
            p->dev.stamps_reg = std::strcmp(sv, "reg") == 0;
        }
        LP_HIP(ctx, hipEventRecord(p->ev0, ctx->stream));
        int rc = lp_batched_launch(ctx, p->dev);
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
        rc = lp_simplex_run(p->lps[(size_t)k], eps, max_iter, LP_SIMPLEX_ALGO_AUTO, &st);
        if (rc < 0) return rc;
        p->status[(size_t)k] = rc;
        p->iters[(size_t)k] = st.pivots;
        total += st.solve_ms;
    }
    if (ms_out) *ms_out = total;
    return LP_OPTIMAL;
}

int lp_batched_download(lp_batched_problem* p, double* x_out, int* basis_out, double* obj_out,
                        int* iters_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
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
    lp_batched_problem* p = nullptr;
    int rc = lp_batched_upload(ctx, batch, A, m, n, b, c, basis_in, maximize, n_orig, &p);
    if (rc) return rc;
    rc = lp_batched_run(p, eps, max_iter, nullptr);
    if (rc == LP_OPTIMAL) rc = lp_batched_download(p, x_out, basis_out, obj_out, iters_out, status_out);
    lp_batched_free(p);
    return rc;
}

}  // extern "C"
