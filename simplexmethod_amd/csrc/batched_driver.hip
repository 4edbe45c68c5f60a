// batched_driver.hip — the host side of the batch handle (lp_batched_problem, batched_problem.hpp) and of the
// bounded-variable simplex.  A handle is of one of three kinds: plain (from given bases, batched_simplex.hip),
// two-phase (no starting basis, batched_two_phase.hip) and re-solve (primal or dual simplex from given bases,
// batched_resolve.hip).  The three upload entries check their arguments and decide `resident`; everything after
// that is written once: batched_upload, run_resident / run_per_lp behind lp_batched_run, and lp_batched_download.
// A resident handle runs one LP per workgroup; any other handle (a plain batch whose bases are not the slack
// identity, a shape beyond one CU's LDS) goes through the single-LP entries of simplex_driver.hip one LP after
// another and keeps each LP's results on the host.  The bounded-variable simplex (batched_bounded.hip) and its re-solve
// from given bases (batched_bounded_resolve.hip) have no handle and no fallback: bounded_solve uploads, launches and
// downloads in one call; the branch-and-bound over the bounds (batched_mip_bounded.hip) does the same through
// mip_bounded_solve and shares bounded_args and bounded_upload.
#include <chrono>
#include <cmath>
#include <memory>

#include "batched_problem.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

// x.head(n_orig) (SimplexSolover.h:435-438) and Canonical::Evaluate (Canonical.cpp:86: c.x over all n columns in
// index order) of one LP's full vertex; either output may be null.
static void finish_x_obj(const double* x, const double* c, int n, int n_orig, double* x_out, double* obj_out) {
    if (x_out)
        for (int j = 0; j < n_orig; ++j) x_out[j] = x[j];
    if (obj_out) {
        double z = 0.0;
        for (int j = 0; j < n; ++j) z += c[j] * x[j];
        *obj_out = z;
    }
}

extern "C" void lp_batched_free(lp_batched_problem* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    for (auto* q : p->lps) lp_simplex_free(q);
    (void)hipFree(p->arena);
    (void)hipFree(p->dstamps);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    delete p;
}

// ===========================================================================
// upload
// ===========================================================================

// The handle of `batch` checked LPs.  A resident handle's inputs and outputs live in one device allocation; any
// other handle keeps the inputs on the host (the run's, and lp_batched_duals' and its siblings'), and a plain one
// uploads every LP as a single-LP problem.  basis_in: nullptr for a two-phase batch.
static int batched_upload(lp_context* ctx, lp_batched_kind kind, bool resident, int pitch, int batch, const double* A,
                          int m, int n, const double* b, const double* c, const int* basis_in, int maximize,
                          int n_orig, lp_batched_problem** problem_out) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<lp_batched_problem, void (*)(lp_batched_problem*)> owner(new lp_batched_problem(), lp_batched_free);
    lp_batched_problem* p = owner.get();   // (freed with everything it holds on every failed return)
    const size_t B = (size_t)batch;
    p->ctx = ctx;
    p->kind = kind;
    p->batch = batch;
    p->m = m;
    p->n = n;
    p->n_orig = n_orig;
    p->maximize = maximize ? 1 : 0;
    p->iter_width = kind == LP_BATCHED_TWO_PHASE ? 3 : kind == LP_BATCHED_RESOLVE ? 2 : 1;
    p->resident = resident;
    p->pitch = pitch;
    p->status.assign(B, -100);
    p->iters.assign(B * p->iter_width, 0);
    p->h_c.assign(c, c + B * n);
    if (!resident) {
        p->h_A.assign(A, A + B * m * n);
        p->h_b.assign(b, b + B * m);
        p->h_x.assign(B * n_orig, 0.0);
        p->h_obj.assign(B, 0.0);
        p->h_basis.assign(B * m, -1);
        if (basis_in) p->h_basis_in.assign(basis_in, basis_in + B * m);
        if (basis_in) p->h_basis = p->h_basis_in;
        for (size_t k = 0; kind == LP_BATCHED_PLAIN && k < B; ++k) {
            lp_simplex_problem* q = nullptr;
            const int rc = lp_simplex_upload(ctx, A + k * m * n, m, n, b + k * m, c + k * n, basis_in + k * m,
                                             maximize, n_orig, &q);
            if (rc) return rc;
            p->lps.push_back(q);
        }
        *problem_out = owner.release();
        return LP_OPTIMAL;
    }
    const size_t szA = sizeof(double) * B * m * n, szb = sizeof(double) * B * m, szc = sizeof(double) * B * n,
                 szbasis = sizeof(int) * B * m;
    // A first; every later piece starts 16-byte aligned, which is enough: the batched kernels read and write these
    // arrays with scalar 8-byte (and 4-byte) accesses only
    hipError_t e = lp_carve_malloc(&p->arena, [&](lp_carver& cut) {
        p->dA = cut.take<double>(szA);
        p->db = cut.take<double>(szb);
        p->dc = cut.take<double>(szc);
        p->dx = cut.take<double>(szc);
        p->dbasis_in = basis_in ? cut.take<int>(szbasis) : nullptr;
        p->dbasis_out = cut.take<int>(szbasis);
        p->diters = cut.take<int>(sizeof(int) * B * p->iter_width);
        p->dstatus = cut.take<int>(sizeof(int) * B);
    });
    hipStream_t s = ctx->stream;
    if (e == hipSuccess) e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
    if (e == hipSuccess) e = hipMemcpyAsync(p->dA, A, szA, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->db, b, szb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->dc, c, szc, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && basis_in) e = hipMemcpyAsync(p->dbasis_in, basis_in, szbasis, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched upload: ") + hipGetErrorString(e));
    *problem_out = owner.release();
    return LP_OPTIMAL;
}

// check_canonical for every LP of a batch with bases.
static int check_batch(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                       const int* basis_in, int n_orig) {
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    for (int k = 0; k < batch; ++k) {
        const int rc = check_canonical(ctx, A ? A + (size_t)k * m * n : nullptr, m, n, b ? b + (size_t)k * m : nullptr,
                                       c ? c + (size_t)k * n : nullptr, basis_in ? basis_in + (size_t)k * m : nullptr,
                                       n_orig);
        if (rc) return rc;
    }
    return LP_OPTIMAL;
}

extern "C" {

int lp_batched_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                      const int* basis_in, int maximize, int n_orig, lp_batched_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    const int rc = check_batch(ctx, batch, A, m, n, b, c, basis_in, n_orig);
    if (rc) return rc;
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
    return batched_upload(ctx, LP_BATCHED_PLAIN, identity && lds <= 160 * 1024, pitch, batch, A, m, n, b, c, basis_in,
                          maximize, n_orig, problem_out);
}

int lp_batched_two_phase_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                const double* c, int maximize, int n_orig, lp_batched_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    // the checks of lp_simplex_two_phase
    if (!A || !b || !c) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_two_phase_upload: null argument");
    if (m <= 0 || n < m || n_orig <= 0 || n_orig > n)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_two_phase_upload: bad dimensions");
    int pitch = 0;
    (void)lp_batched_two_phase_lds_bytes(m, n, &pitch);
    return batched_upload(ctx, LP_BATCHED_TWO_PHASE, lp_batched_two_phase_fits(m, n), pitch, batch, A, m, n, b, c,
                          nullptr, maximize, n_orig, problem_out);
}

int lp_batched_resolve_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                              const double* c, const int* basis_in, int maximize, int n_orig,
                              lp_batched_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    const int rc = check_batch(ctx, batch, A, m, n, b, c, basis_in, n_orig);
    if (rc) return rc;
    int pitch = 0;
    (void)lp_batched_two_phase_lds_bytes(m, n, &pitch);
    return batched_upload(ctx, LP_BATCHED_RESOLVE, lp_batched_two_phase_fits(m, n), pitch, batch, A, m, n, b, c,
                          basis_in, maximize, n_orig, problem_out);
}

int lp_batched_set_start(lp_batched_problem* p, const double* b, const int* basis_in) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (p->kind != LP_BATCHED_RESOLVE) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_set_start: not a re-solve batch");
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

int lp_batched_set_pivot_rule(lp_batched_problem* p, int pivot_rule) {
    if (!p) return LP_BAD_ARG;
    if (!lp_pivot_rule_known(pivot_rule))
        LP_FAIL(p->ctx, LP_BAD_ARG, "unknown pivot rule");
    p->pivot_rule = pivot_rule;
    return LP_OPTIMAL;
}

int lp_batched_devex_fits(int m, int n, int two_phase) {
    if (m <= 0 || n < m) return 0;
    if (two_phase) return lp_batched_two_phase_devex_lds_bytes(m, n) <= 160 * 1024 ? 1 : 0;
    return n > m && lp_batched_devex_lds_bytes(m, n) <= 160 * 1024 ? 1 : 0;
}

int lp_batched_shard_bounds(int batch, int shard, int shards, int* lo, int* hi) {
    if (batch < 0 || shards < 1 || shard < 0 || shard >= shards || !lo || !hi) return LP_BAD_ARG;
    *lo = (int)((long long)batch * shard / shards);
    *hi = (int)((long long)batch * (shard + 1) / shards);
    return LP_OPTIMAL;
}

int lp_batched_path(const lp_batched_problem* p) {
    if (!p) return LP_BAD_ARG;
    return p->resident ? 1 : 0;
}

}  // extern "C"

// ===========================================================================
// run
// ===========================================================================

// The fields every kind's kernel argument has, from the handle.
template <typename Dev>
static Dev dev_args(const lp_batched_problem* p, double eps, int max_iter) {
    Dev d{};
    d.batch = p->batch;
    d.m = p->m;
    d.n = p->n;
    d.pitch = p->pitch;
    d.maximize = p->maximize;
    d.max_iter = max_iter;
    d.eps = eps;
    d.A = p->dA;
    d.b = p->db;
    d.c = p->dc;
    d.x = p->dx;
    d.basis_out = p->dbasis_out;
    d.iters = p->diters;
    d.status = p->dstatus;
    return d;
}

static int launch(lp_batched_problem* p, double eps, int max_iter) {
    switch (p->kind) {
        case LP_BATCHED_TWO_PHASE:
            return lp_batched_two_phase_launch(p->ctx, dev_args<BatchedTwoPhaseDev>(p, eps, max_iter), p->pivot_rule);
        case LP_BATCHED_RESOLVE: {
            BatchedResolveDev d = dev_args<BatchedResolveDev>(p, eps, max_iter);
            d.basis_in = p->dbasis_in;
            return lp_batched_resolve_launch(p->ctx, d);
        }
        default: {
            BatchedDev d = dev_args<BatchedDev>(p, eps, max_iter);
            d.basis_in = p->dbasis_in;
            d.stamps = p->dstamps;
            d.stamps_reg = p->stamps_reg;
            return lp_batched_launch(p->ctx, d, p->pivot_rule);
        }
    }
}

// LP_BATCHED_STAMPS: the diagnostic build of the plain kernel (scripts/stamp_batched.py); the buffer holds 32 phase
// sums + 2 per wave (16 waves).
static int stamps_prepare(lp_batched_problem* p) {
    const char* sv = getenv("LP_BATCHED_STAMPS");
    if (!sv || p->dstamps || p->kind != LP_BATCHED_PLAIN) return LP_OPTIMAL;
    LP_HIP(p->ctx, hipMalloc(&p->dstamps, sizeof(unsigned long long) * 64));
    LP_HIP(p->ctx, hipMemset(p->dstamps, 0, sizeof(unsigned long long) * 64));
    p->stamps_reg = std::strcmp(sv, "reg") == 0;
    return LP_OPTIMAL;
}

static int stamps_print(lp_batched_problem* p, float ms) {
    unsigned long long h[64];
    LP_HIP(p->ctx, hipMemcpy(h, p->dstamps, sizeof(h), hipMemcpyDeviceToHost));
    if (p->stamps_reg) {
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
    return LP_OPTIMAL;
}

// One launch of the kind's kernel over the whole batch, timed by device events.
static int run_resident(lp_batched_problem* p, double eps, int max_iter, float* ms_out) {
    lp_context* ctx = p->ctx;
    int rc = stamps_prepare(p);
    if (rc) return rc;
    LP_HIP(ctx, hipEventRecord(p->ev0, ctx->stream));
    rc = launch(p, eps, max_iter);
    if (rc) return rc;
    LP_HIP(ctx, hipGetLastError());
    LP_HIP(ctx, hipEventRecord(p->ev1, ctx->stream));
    LP_HIP(ctx, hipEventSynchronize(p->ev1));
    float ms = 0.f;
    LP_HIP(ctx, hipEventElapsedTime(&ms, p->ev0, p->ev1));
    if (ms_out) *ms_out = ms;
    return p->dstamps ? stamps_print(p, ms) : LP_OPTIMAL;
}

// The per-LP fallback: the kind's single-LP solve one LP after another.  Each LP's status, pivot counts and final
// basis, and for LP_OPTIMAL its x and obj, go to the handle's host arrays.  ms_out: the sum of the solves' own times
// for a plain batch, the host clock over the loop for the other two.
static int run_per_lp(lp_batched_problem* p, double eps, int max_iter, float* ms_out) {
    lp_context* ctx = p->ctx;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t m = (size_t)p->m, n = (size_t)p->n, no = (size_t)p->n_orig;
    float solve_ms = 0.f;
    for (size_t k = 0; k < (size_t)p->batch; ++k) {
        const double *Ak = p->h_A.data() + k * m * n, *bk = p->h_b.data() + k * m, *ck = p->h_c.data() + k * n;
        double *xk = p->h_x.data() + k * no, *objk = p->h_obj.data() + k;
        int *basisk = p->h_basis.data() + k * m, *itk = p->iters.data() + k * p->iter_width;
        lp_simplex_problem* q = nullptr;   // the two kinds that solve through a single-LP problem
        int rc;
        switch (p->kind) {
            case LP_BATCHED_TWO_PHASE:
                rc = lp_simplex_two_phase_ex(ctx, Ak, p->m, p->n, bk, ck, p->maximize, p->n_orig, eps, max_iter, xk,
                                             basisk, objk, itk, p->pivot_rule);
                if (rc > LP_INFEASIBLE) return rc;
                break;
            case LP_BATCHED_RESOLVE:
                rc = lp_simplex_upload(ctx, Ak, p->m, p->n, bk, ck, p->h_basis_in.data() + k * m, p->maximize,
                                       p->n_orig, &q);
                if (rc) return rc;
                rc = lp_simplex_resolve_run(q, eps, max_iter, itk, nullptr);
                break;
            default: {
                q = p->lps[k];
                rc = lp_simplex_reset(q);
                if (rc) return rc;
                q->pivot_rule = p->pivot_rule;
                lp_simplex_stats st;
                rc = lp_simplex_run(q, eps, max_iter, LP_SIMPLEX_ALGO_AUTO, &st);
                if (rc >= 0) {
                    itk[0] = st.pivots;
                    solve_ms += st.solve_ms;
                }
            }
        }
        if (q && rc >= 0) {
            const bool ok = rc == LP_OPTIMAL;
            const int drc = lp_simplex_download(q, ok ? xk : nullptr, basisk, ok ? objk : nullptr, nullptr, nullptr, 0,
                                                nullptr);
            if (drc) rc = drc;
        }
        if (p->kind == LP_BATCHED_RESOLVE) lp_simplex_free(q);
        if (rc < 0) return rc;
        p->status[k] = rc;
    }
    if (p->kind == LP_BATCHED_RESOLVE) ctx->last_error.clear();   // (a basis that is no valid start is a per-LP status here)
    if (ms_out)
        *ms_out = p->kind == LP_BATCHED_PLAIN
                      ? solve_ms
                      : std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return LP_OPTIMAL;
}

extern "C" int lp_batched_run(lp_batched_problem* p, double eps, int max_iter, float* ms_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_run: eps must be >= 0");
    p->ran = false;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (p->kind == LP_BATCHED_RESOLVE && p->pivot_rule != LP_PIVOT_DANTZIG)
        LP_FAIL(ctx, LP_BAD_ARG, "the re-solve runs Dantzig's rule only");
    const int rc = p->resident ? run_resident(p, eps, max_iter, ms_out) : run_per_lp(p, eps, max_iter, ms_out);
    p->ran = rc == LP_OPTIMAL;
    return rc;
}

// ===========================================================================
// download
// ===========================================================================

extern "C" int lp_batched_download(lp_batched_problem* p, double* x_out, int* basis_out, double* obj_out,
                                   int* iters_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)p->batch, m = (size_t)p->m, n = (size_t)p->n, no = (size_t)p->n_orig, w = (size_t)p->iter_width;
    std::vector<double> x;   // a resident handle's full vertices
    if (p->resident) {
        x.resize(B * n);
        const int rc = lp_download(ctx, "batched download", {{x.data(), p->dx, sizeof(double) * B * n},
                                                             {p->status.data(), p->dstatus, sizeof(int) * B},
                                                             {p->iters.data(), p->diters, sizeof(int) * B * w},
                                                             {basis_out, p->dbasis_out, basis_out ? sizeof(int) * B * m : 0}});
        if (rc) return rc;
    } else if (basis_out) {
        std::memcpy(basis_out, p->h_basis.data(), sizeof(int) * B * m);
    }
    for (size_t k = 0; k < B; ++k) {
        if (p->status[k] == LP_OPTIMAL) {
            double* xk = x_out ? x_out + k * no : nullptr;
            if (p->resident) {
                finish_x_obj(x.data() + k * n, p->h_c.data() + k * n, p->n, p->n_orig, xk, obj_out ? obj_out + k : nullptr);
            } else {
                if (xk) std::memcpy(xk, p->h_x.data() + k * no, sizeof(double) * no);
                if (obj_out) obj_out[k] = p->h_obj[k];
            }
        }
        if (iters_out) {
            iters_out[k] = 0;
            for (size_t j = 0; j < w; ++j) iters_out[k] += p->iters[k * w + j];
        }
        if (status_out) status_out[k] = p->status[k];
    }
    return LP_OPTIMAL;
}

// The pivot counts of the last run, iter_width per LP, of a handle of the given kind.
static int batched_counters(lp_batched_problem* p, lp_batched_kind kind, const char* refusal, int* iters_out) {
    if (!p || !iters_out) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (p->kind != kind) LP_FAIL(ctx, LP_BAD_ARG, refusal);
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(int) * (size_t)p->batch * p->iter_width;
    if (p->resident) {
        const int rc = lp_download(ctx, "batched pivot counts", {{p->iters.data(), p->diters, bytes}});
        if (rc) return rc;
    }
    std::memcpy(iters_out, p->iters.data(), bytes);
    return LP_OPTIMAL;
}

// ===========================================================================
// one-shot entries: upload, run, download, free
// ===========================================================================

// iters_out: the handle's pivot counts, iter_width per LP (download has brought a resident handle's to the host).
static int solve_and_free(lp_batched_problem* p, int pivot_rule, double eps, int max_iter, double* x_out,
                          int* basis_out, double* obj_out, int* iters_out, int* status_out) {
    p->pivot_rule = pivot_rule;
    int rc = lp_batched_run(p, eps, max_iter, nullptr);
    if (rc == LP_OPTIMAL) rc = lp_batched_download(p, x_out, basis_out, obj_out, nullptr, status_out);
    if (rc == LP_OPTIMAL && iters_out) std::memcpy(iters_out, p->iters.data(), sizeof(int) * p->iters.size());
    lp_batched_free(p);
    return rc;
}

extern "C" {

int lp_batched_phase_iters(lp_batched_problem* p, int* iters_out) {
    return batched_counters(p, LP_BATCHED_TWO_PHASE, "lp_batched_phase_iters: not a two-phase batch", iters_out);
}

int lp_batched_resolve_iters(lp_batched_problem* p, int* iters_out) {
    return batched_counters(p, LP_BATCHED_RESOLVE, "lp_batched_resolve_iters: not a re-solve batch", iters_out);
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
    if (ctx && !lp_pivot_rule_known(pivot_rule))
        LP_FAIL(ctx, LP_BAD_ARG, "unknown pivot rule");
    if (ctx && !(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_solve_batched: eps must be >= 0");
    lp_batched_problem* p = nullptr;
    const int rc = lp_batched_upload(ctx, batch, A, m, n, b, c, basis_in, maximize, n_orig, &p);
    if (rc) return rc;
    return solve_and_free(p, pivot_rule, eps, max_iter, x_out, basis_out, obj_out, iters_out, status_out);
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
    if (!lp_pivot_rule_known(pivot_rule)) LP_FAIL(ctx, LP_BAD_ARG, "unknown pivot rule");
    lp_batched_problem* p = nullptr;
    const int rc = lp_batched_two_phase_upload(ctx, batch, A, m, n, b, c, maximize, n_orig, &p);
    if (rc) return rc;
    return solve_and_free(p, pivot_rule, eps, max_iter, x_out, basis_out, obj_out, iters_out, status_out);
}

int lp_simplex_resolve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                               const double* c, const int* basis_in, int maximize, int n_orig, double eps,
                               int max_iter, double* x_out, int* basis_out, double* obj_out, int* iters_out,
                               int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_resolve_batched: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_resolve_batched: eps must be >= 0");
    lp_batched_problem* p = nullptr;
    const int rc = lp_batched_resolve_upload(ctx, batch, A, m, n, b, c, basis_in, maximize, n_orig, &p);
    if (rc) return rc;
    return solve_and_free(p, LP_PIVOT_DANTZIG, eps, max_iter, x_out, basis_out, obj_out, iters_out, status_out);
}

}  // extern "C"

// ===========================================================================
// Bounded-variable simplex (batched_bounded.hip) and its re-solve from given bases (batched_bounded_resolve.hip): one LP
// per workgroup for lp_simplex_bounded_fits shapes only; there is no handle and no per-LP host fallback
// ===========================================================================

// The checks of the entry points: pointers, dimensions, the bounds of every LP (lo finite, hi not NaN) and the fit; for
// a re-solve (warm) also the start of every LP: basis indices in [0, n), flags 0 or 1, and 1 only under a finite hi.
static int bounded_args(lp_context* ctx, const char* who, int batch, const double* A, int m, int n, const double* b,
                        const double* c, const double* lo, const double* hi, int n_orig, bool warm = false,
                        const int* basis_in = nullptr, const int* at_upper_in = nullptr) {
    if (!A || !b || !c || !lo || !hi || (warm && (!basis_in || !at_upper_in)))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (m <= 0 || n < m || n_orig <= 0 || n_orig > n) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    const size_t N = (size_t)batch * n;
    for (size_t j = 0; j < N; ++j) {
        if (!std::isfinite(lo[j])) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": lo must be finite");
        if (std::isnan(hi[j])) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": hi is NaN");
        if (!warm) continue;
        if (at_upper_in[j] != 0 && at_upper_in[j] != 1) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": at_upper must be 0 or 1");
        if (at_upper_in[j] && std::isinf(hi[j]))
            LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": a column without an upper bound is flagged at_upper");
    }
    for (size_t t = 0; warm && t < (size_t)batch * m; ++t)
        if (basis_in[t] < 0 || basis_in[t] >= n) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": basis index out of range");
    if (!lp_bounded_fits_shape(m, n))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the shape does not fit one CU's LDS (lp_simplex_bounded_fits)");
    return LP_OPTIMAL;
}

// The inputs of `batch` bounded LPs on the device: one allocation, the doubles first.  out_d / out_i: room for the
// caller's outputs (and further int inputs) behind them.
struct BoundedInputs {
    double *A, *b, *c, *lo, *hi, *out_d;
    int *basis_in, *at_upper_in, *out_i;   // the first two: nullptr without a start
};

// Allocates and queues the uploads (the start too when basis_in is given); the launch that follows on the context's
// stream orders itself behind them.
static int bounded_upload(lp_context* ctx, lp_device_buffer& buf, int batch, const double* A, int m, int n,
                          const double* b, const double* c, const double* lo, const double* hi, const int* basis_in,
                          const int* at_upper_in, size_t out_doubles, size_t out_ints, BoundedInputs& in) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch;
    const size_t dbl = B * ((size_t)m * n + m + 3 * (size_t)n) + out_doubles;
    const size_t ints = (basis_in ? B * ((size_t)m + n) : 0) + out_ints;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * dbl + sizeof(int) * ints));
    in.A = reinterpret_cast<double*>(buf.ptr);
    in.b = in.A + B * m * n;
    in.c = in.b + B * m;
    in.lo = in.c + B * n;
    in.hi = in.lo + B * n;
    in.out_d = in.hi + B * n;
    int* ip = reinterpret_cast<int*>(in.out_d + out_doubles);
    in.basis_in = basis_in ? ip : nullptr;
    in.at_upper_in = basis_in ? ip + B * m : nullptr;
    in.out_i = basis_in ? ip + B * ((size_t)m + n) : ip;
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(in.A, A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(in.b, b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(in.c, c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(in.lo, lo, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(in.hi, hi, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && basis_in) e = hipMemcpyAsync(in.basis_in, basis_in, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && basis_in) e = hipMemcpyAsync(in.at_upper_in, at_upper_in, sizeof(int) * B * n, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched bounded simplex upload: ") + hipGetErrorString(e));
    return LP_OPTIMAL;
}

// Uploads `batch` LPs, runs k_batched_bounded (basis_in null: 4 counters per LP) or k_batched_bounded_resolve (from
// basis_in and at_upper_in: 3 counters per LP) and downloads; x (n_orig) and obj (over all n columns, as
// lp_simplex_two_phase_batched) are written for LP_OPTIMAL LPs only.  pivot_rule picks the kernel's rule form (the
// re-solve: of its primal branch); LP_PIVOT_DANTZIG is the kernel the entries without _ex launch.  dual_rule (the
// re-solve only) picks the pricing of its dual branch; LP_DUAL_DANTZIG is the kernel the _ex entries launch.  dual_ratio
// (the re-solve only) picks that branch's ratio test; LP_DUAL_RATIO_TEXTBOOK is the kernel the _dual_ex entries launch.
static int bounded_solve(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                         const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize,
                         int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out,
                         double* obj_out, int* iters_out, int* status_out, int pivot_rule = LP_PIVOT_DANTZIG,
                         int dual_rule = LP_DUAL_DANTZIG, int dual_ratio = LP_DUAL_RATIO_TEXTBOOK) {
    const size_t B = (size_t)batch, iw = basis_in ? 3 : 4;
    lp_device_buffer buf;
    BoundedInputs in;
    int rc = bounded_upload(ctx, buf, batch, A, m, n, b, c, lo, hi, basis_in, at_upper_in, B * n,
                            B * ((size_t)m + n + iw + 1), in);
    if (rc) return rc;
    BatchedBoundedResolveDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    (void)lp_bounded_lds_bytes(m, n, &d.pitch);
    d.maximize = maximize ? 1 : 0;
    d.max_iter = max_iter;
    d.eps = eps;
    d.A = in.A;
    d.b = in.b;
    d.c = in.c;
    d.lo = in.lo;
    d.hi = in.hi;
    d.x = in.out_d;
    d.basis_out = in.out_i;
    d.at_upper = d.basis_out + B * m;
    d.iters = d.at_upper + B * n;
    d.status = d.iters + B * iw;
    d.basis_in = in.basis_in;
    d.at_upper_in = in.at_upper_in;
    std::vector<double> x(B * n);
    rc = basis_in ? lp_batched_bounded_resolve_launch(ctx, d, pivot_rule, dual_rule, dual_ratio) : lp_batched_bounded_launch(ctx, d, pivot_rule);
    if (rc) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched bounded simplex: ") + hipGetErrorString(e));
    rc = lp_download(ctx, "batched bounded simplex", {{x.data(), d.x, sizeof(double) * B * n},
                                                      {basis_out, d.basis_out, sizeof(int) * B * m},
                                                      {at_upper_out, d.at_upper, sizeof(int) * B * n},
                                                      {iters_out, d.iters, sizeof(int) * B * iw},
                                                      {status_out, d.status, sizeof(int) * B}});
    if (rc) return rc;
    for (size_t k = 0; k < B; ++k)
        if (status_out[k] == LP_OPTIMAL) finish_x_obj(x.data() + k * n, c + k * n, n, n_orig, x_out + k * n_orig, obj_out + k);
    return LP_OPTIMAL;
}

// Branch-and-bound over the bounds (batched_mip_bounded.hip): the checks of the bounded re-solve and of the search
// (lp_mip_check_search, basis_driver.hip), integral bounds on the marked columns, and the fit.
static int mip_bounded_args(lp_context* ctx, const char* who, int batch, const double* A, int m, int n, const double* b,
                            const double* c, const double* lo, const double* hi, const int* basis_in,
                            const int* at_upper_in, int n_orig, const int* integer, double int_tol, double gap,
                            int max_depth, int max_nodes) {
    int rc = bounded_args(ctx, who, batch, A, m, n, b, c, lo, hi, n_orig, true, basis_in, at_upper_in);
    if (rc) return rc;
    rc = lp_mip_check_search(ctx, who, n, n_orig, integer, int_tol, gap, max_depth, LP_MIP_BOUNDED_MAX_DEPTH, max_nodes);
    if (rc) return rc;
    for (size_t k = 0; k < (size_t)batch; ++k)
        for (int j = 0; j < n_orig; ++j) {
            const double l = lo[k * n + j], h = hi[k * n + j];
            if (integer[j] && (l != std::floor(l) || (std::isfinite(h) && h != std::floor(h))))
                LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": an integer column has a fractional bound");
        }
    if (!lp_mip_bounded_fits_shape(m, n, max_depth))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the shape does not fit one CU's LDS (lp_mip_bounded_fits)");
    return LP_OPTIMAL;
}

// Uploads `batch` problems with their starts, the mask and root_status (may be null), runs k_batched_mip_bounded (its
// _long form under LP_DUAL_RATIO_LONG_STEP) and downloads.
static int mip_bounded_solve(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                             const double* c, const double* lo, const double* hi, const int* basis_in,
                             const int* at_upper_in, const int* root_status, int maximize, int n_orig,
                             const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes,
                             int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out,
                             int* stats_out, int* status_out, int dual_ratio) {
    const size_t B = (size_t)batch;
    lp_device_buffer buf;
    BoundedInputs in;
    int rc = bounded_upload(ctx, buf, batch, A, m, n, b, c, lo, hi, basis_in, at_upper_in, B * ((size_t)n_orig + 2),
                            B * 8 + n, in);
    if (rc) return rc;
    BatchedMipBoundedDev d{};
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
    d.A = in.A;
    d.b = in.b;
    d.c = in.c;
    d.lo = in.lo;
    d.hi = in.hi;
    d.basis_in = in.basis_in;
    d.at_upper_in = in.at_upper_in;
    d.x = in.out_d;
    d.obj = d.x + B * n_orig;
    d.bound = d.obj + B;
    d.found = in.out_i;
    d.stats = d.found + B;
    d.status = d.stats + B * 5;
    int* droot = d.status + B;
    int* dmask = droot + B;
    d.root_status = root_status ? droot : nullptr;
    d.integer = dmask;
    hipError_t e = hipMemcpyAsync(dmask, integer, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && root_status)
        e = hipMemcpyAsync(droot, root_status, sizeof(int) * B, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched bounded MIP upload: ") + hipGetErrorString(e));
    rc = lp_batched_mip_bounded_launch(ctx, d, dual_ratio);
    if (rc) return rc;
    e = hipGetLastError();
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched bounded MIP: ") + hipGetErrorString(e));
    return lp_download(ctx, "batched bounded MIP", {{x_out, d.x, sizeof(double) * B * n_orig},
                                                    {obj_out, d.obj, sizeof(double) * B},
                                                    {bound_out, d.bound, sizeof(double) * B},
                                                    {found_out, d.found, sizeof(int) * B},
                                                    {stats_out, d.stats, sizeof(int) * B * 5},
                                                    {status_out, d.status, sizeof(int) * B}});
}

// The rule check of the bounded _ex entries: a known rule, and under Devex room for the weights too.  Nothing is
// launched on a refusal.
static int bounded_rule_args(lp_context* ctx, const char* who, int m, int n, int pivot_rule) {
    if (!lp_pivot_rule_known(pivot_rule)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": unknown pivot rule");
    if (!lp_bounded_rule_fits_shape(m, n, pivot_rule))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the tableau and the Devex weights do not fit one CU's LDS (lp_simplex_bounded_rule_fits)");
    return LP_OPTIMAL;
}

// The eight entries of the family in one: single (batch 1, status_out null: the status is the return value) or
// batched, cold or from given bases (warm), under pivot_rule.  The entries without _ex pass LP_PIVOT_DANTZIG.  The two
// _dual_ex entries (warm) pass dual_rule too: an unknown one is refused before anything else is looked at, and Devex
// needs room for the larger of the two weight arrays (lp_simplex_bounded_dual_rule_fits).  The two _ratio_ex entries
// (warm) pass dual_ratio as well: an unknown one is refused ahead of even that; the long-step form needs no LDS more.
static int bounded_entry(lp_context* ctx, const char* who, bool batched, bool warm, int batch, const double* A, int m,
                         int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in,
                         const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                         int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out,
                         int pivot_rule, int dual_rule = LP_DUAL_DANTZIG, int dual_ratio = LP_DUAL_RATIO_TEXTBOOK) {
    if (!ctx) return LP_BAD_ARG;
    if (!lp_dual_ratio_known(dual_ratio)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": unknown dual ratio test");
    if (!lp_dual_rule_known(dual_rule)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": unknown dual rule");
    if (!x_out || !basis_out || !at_upper_out || !obj_out || !iters_out || (batched && !status_out))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": eps must be >= 0");
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    int rc = bounded_args(ctx, who, batch, A, m, n, b, c, lo, hi, n_orig, warm, basis_in, at_upper_in);
    if (rc) return rc;
    rc = bounded_rule_args(ctx, who, m, n, pivot_rule);
    if (rc) return rc;
    if (!lp_bounded_dual_rule_fits_shape(m, n, pivot_rule, dual_rule))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the tableau and the Devex weights do not fit one CU's LDS (lp_simplex_bounded_dual_rule_fits)");
    int status = LP_OPTIMAL;
    rc = bounded_solve(ctx, batch, A, m, n, b, c, lo, hi, warm ? basis_in : nullptr, warm ? at_upper_in : nullptr,
                       maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out,
                       batched ? status_out : &status, pivot_rule, dual_rule, dual_ratio);
    if (rc || batched) return rc;
    if (warm && status == LP_BAD_ARG)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the basis is neither primal nor dual feasible");
    return status;
}

extern "C" {

int lp_simplex_bounded_fits(int m, int n) { return lp_bounded_fits_shape(m, n) ? 1 : 0; }

int lp_simplex_bounded(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo,
                       const double* hi, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                       int* basis_out, int* at_upper_out, double* obj_out, int* iters_out) {
    return bounded_entry(ctx, "lp_simplex_bounded", false, false, 1, A, m, n, b, c, lo, hi, nullptr, nullptr,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, nullptr,
                         LP_PIVOT_DANTZIG);
}

int lp_simplex_bounded_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                               const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter,
                               double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out) {
    return bounded_entry(ctx, "lp_simplex_bounded_batched", true, false, batch, A, m, n, b, c, lo, hi, nullptr, nullptr,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, status_out,
                         LP_PIVOT_DANTZIG);
}

int lp_simplex_bounded_resolve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo,
                               const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                               int* basis_out, int* at_upper_out, double* obj_out, int* iters_out) {
    return bounded_entry(ctx, "lp_simplex_bounded_resolve", false, true, 1, A, m, n, b, c, lo, hi, basis_in, at_upper_in,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, nullptr,
                         LP_PIVOT_DANTZIG);
}

int lp_simplex_bounded_resolve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                                       const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter,
                                       double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out) {
    return bounded_entry(ctx, "lp_simplex_bounded_resolve_batched", true, true, batch, A, m, n, b, c, lo, hi, basis_in, at_upper_in,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, status_out,
                         LP_PIVOT_DANTZIG);
}

int lp_simplex_bounded_rule_fits(int m, int n, int pivot_rule) { return lp_bounded_rule_fits_shape(m, n, pivot_rule) ? 1 : 0; }

int lp_simplex_bounded_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo,
                          const double* hi, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                          int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule) {
    return bounded_entry(ctx, "lp_simplex_bounded_ex", false, false, 1, A, m, n, b, c, lo, hi, nullptr, nullptr,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, nullptr,
                         pivot_rule);
}

int lp_simplex_bounded_batched_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                                  const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter,
                                  double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out, int pivot_rule) {
    return bounded_entry(ctx, "lp_simplex_bounded_batched_ex", true, false, batch, A, m, n, b, c, lo, hi, nullptr, nullptr,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, status_out,
                         pivot_rule);
}

int lp_simplex_bounded_resolve_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo,
                                  const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                                  int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule) {
    return bounded_entry(ctx, "lp_simplex_bounded_resolve_ex", false, true, 1, A, m, n, b, c, lo, hi, basis_in, at_upper_in,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, nullptr,
                         pivot_rule);
}

int lp_simplex_bounded_resolve_batched_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                                          const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter,
                                          double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out, int pivot_rule) {
    return bounded_entry(ctx, "lp_simplex_bounded_resolve_batched_ex", true, true, batch, A, m, n, b, c, lo, hi, basis_in, at_upper_in,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, status_out,
                         pivot_rule);
}

int lp_simplex_bounded_dual_rule_fits(int m, int n, int pivot_rule, int dual_rule) {
    return lp_bounded_dual_rule_fits_shape(m, n, pivot_rule, dual_rule) ? 1 : 0;
}

int lp_simplex_bounded_resolve_dual_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo,
                                       const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                                       int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule, int dual_rule) {
    return bounded_entry(ctx, "lp_simplex_bounded_resolve_dual_ex", false, true, 1, A, m, n, b, c, lo, hi, basis_in, at_upper_in,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, nullptr,
                         pivot_rule, dual_rule);
}

int lp_simplex_bounded_resolve_batched_dual_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                                               const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter,
                                               double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out, int pivot_rule, int dual_rule) {
    return bounded_entry(ctx, "lp_simplex_bounded_resolve_batched_dual_ex", true, true, batch, A, m, n, b, c, lo, hi, basis_in, at_upper_in,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, status_out,
                         pivot_rule, dual_rule);
}

int lp_simplex_bounded_resolve_ratio_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo,
                                        const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                                        int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule, int dual_rule, int dual_ratio) {
    return bounded_entry(ctx, "lp_simplex_bounded_resolve_ratio_ex", false, true, 1, A, m, n, b, c, lo, hi, basis_in, at_upper_in,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, nullptr,
                         pivot_rule, dual_rule, dual_ratio);
}

int lp_simplex_bounded_resolve_batched_ratio_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c,
                                                const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter,
                                                double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out, int pivot_rule, int dual_rule,
                                                int dual_ratio) {
    return bounded_entry(ctx, "lp_simplex_bounded_resolve_batched_ratio_ex", true, true, batch, A, m, n, b, c, lo, hi, basis_in, at_upper_in,
                         maximize, n_orig, eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out, status_out,
                         pivot_rule, dual_rule, dual_ratio);
}

int lp_mip_bounded_fits(int m, int n, int max_depth) { return lp_mip_bounded_fits_shape(m, n, max_depth) ? 1 : 0; }

// The search over the bounds in LDS.  The entries without a suffix are the _ratio_ex ones under LP_DUAL_RATIO_TEXTBOOK;
// an unknown dual_ratio is refused before anything else is looked at.
int lp_mip_bounded_solve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                         const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize,
                         int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth,
                         int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out,
                         int* found_out, int* stats_out) {
    return lp_mip_bounded_solve_ratio_ex(ctx, A, m, n, b, c, lo, hi, basis_in, at_upper_in, maximize, n_orig, integer,
                                         eps, int_tol, gap, max_depth, max_nodes, max_iter, x_out, obj_out, bound_out,
                                         found_out, stats_out, LP_DUAL_RATIO_TEXTBOOK);
}

int lp_mip_bounded_solve_ratio_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                  const double* lo, const double* hi, const int* basis_in, const int* at_upper_in,
                                  int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap,
                                  int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out,
                                  double* bound_out, int* found_out, int* stats_out, int dual_ratio) {
    if (!ctx) return LP_BAD_ARG;
    if (!lp_dual_ratio_known(dual_ratio)) LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve: unknown dual ratio test");
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve: eps must be >= 0");
    int rc = mip_bounded_args(ctx, "lp_mip_bounded_solve", 1, A, m, n, b, c, lo, hi, basis_in, at_upper_in, n_orig,
                              integer, int_tol, gap, max_depth, max_nodes);
    if (rc) return rc;
    int status = LP_OPTIMAL;
    rc = mip_bounded_solve(ctx, 1, A, m, n, b, c, lo, hi, basis_in, at_upper_in, nullptr, maximize, n_orig, integer, eps,
                           int_tol, gap, max_depth, max_nodes, max_iter, x_out, obj_out, bound_out, found_out, stats_out,
                           &status, dual_ratio);
    if (rc) return rc;
    if (status == LP_BAD_ARG) LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve: the basis is neither primal nor dual feasible");
    return status;
}

int lp_mip_bounded_solve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                 const double* c, const double* lo, const double* hi, const int* basis_in,
                                 const int* at_upper_in, const int* root_status, int maximize, int n_orig,
                                 const int* integer, double eps, double int_tol, double gap, int max_depth,
                                 int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out,
                                 int* found_out, int* stats_out, int* status_out) {
    return lp_mip_bounded_solve_batched_ratio_ex(ctx, batch, A, m, n, b, c, lo, hi, basis_in, at_upper_in, root_status,
                                                 maximize, n_orig, integer, eps, int_tol, gap, max_depth, max_nodes,
                                                 max_iter, x_out, obj_out, bound_out, found_out, stats_out, status_out,
                                                 LP_DUAL_RATIO_TEXTBOOK);
}

int lp_mip_bounded_solve_batched_ratio_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                          const double* c, const double* lo, const double* hi, const int* basis_in,
                                          const int* at_upper_in, const int* root_status, int maximize, int n_orig,
                                          const int* integer, double eps, double int_tol, double gap, int max_depth,
                                          int max_nodes, int max_iter, double* x_out, double* obj_out,
                                          double* bound_out, int* found_out, int* stats_out, int* status_out,
                                          int dual_ratio) {
    if (!ctx) return LP_BAD_ARG;
    if (!lp_dual_ratio_known(dual_ratio))
        LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve_batched: unknown dual ratio test");
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve_batched: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve_batched: eps must be >= 0");
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    const int rc = mip_bounded_args(ctx, "lp_mip_bounded_solve_batched", batch, A, m, n, b, c, lo, hi, basis_in,
                                    at_upper_in, n_orig, integer, int_tol, gap, max_depth, max_nodes);
    if (rc) return rc;
    return mip_bounded_solve(ctx, batch, A, m, n, b, c, lo, hi, basis_in, at_upper_in, root_status, maximize, n_orig,
                             integer, eps, int_tol, gap, max_depth, max_nodes, max_iter, x_out, obj_out, bound_out,
                             found_out, stats_out, status_out, dual_ratio);
}

}  // extern "C"
