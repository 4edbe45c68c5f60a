// basis_driver.hip — the host side of every analysis that starts from an LP and a basis: the dual solution
// (basis_duals.hip), ranging (basis_ranging.hip), certificates (basis_certificate.hip), the parametric right-hand
// side (basis_parametric.hip), the parametric cost (basis_parametric_cost.hip) and branch-and-bound
// (batched_mip.hip).  Each analysis has three entry points: lp_basis_X (one LP), lp_basis_X_batched (a batch from
// the host) and lp_batched_X (a batch handle after its run).  All three put the inputs on the device (upload, or
// where a resident run left them: batch_inputs) and call X_on_device, which launches the analysis's kernel when the
// shape fits it and otherwise runs its single-LP device path one LP after another (per_lp).
// The analyses of a bounded-variable LP at a basis and flags (basis_bounded.hip, basis_bounded_certificate.hip,
// basis_bounded_parametric.hip) have two entry points each (one LP, a batch from the host) and no per-LP path:
// bounded_sens, bounded_certificate and bounded_parametric upload, launch and download in one call.  The duals and
// ranging of one bounded LP beyond the kernel's fit (lp_basis_bounded_duals_large, lp_basis_bounded_ranging_large) go
// through bounded_sens as well, with lp_basis_bounded_device in place of the launch, and its certificate
// (lp_basis_bounded_certificate_large) through bounded_certificate with lp_basis_bounded_certificate_device.
#include <cmath>
#include <functional>

#include "batched_problem.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

// Device pointers to the inputs of a batch.
struct BasisInputs {
    const double *A = nullptr, *b = nullptr, *c = nullptr;
    const int* basis = nullptr;
    const int* run_status = nullptr;   // nullptr: every LP is taken as it is
    const double* extra = nullptr;     // d (m per LP) or g (n per LP) of the parametric analyses
};

// One allocation held by `buf` for the non-null host arrays among A, b, c, `extra` (extra_len doubles per LP), the
// bases and the run statuses; the copies are queued, then one sync.  Sets the device pointers of what went up.
static int upload(lp_context* ctx, const char* what, lp_device_buffer& buf, int batch, int m, int n,
                  const double* A, const double* b, const double* c, const double* extra, size_t extra_len,
                  const int* basis, const int* run_status, BasisInputs& in) {
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch;
    struct Part {
        const void* host;
        size_t bytes;
    };
    const Part parts[6] = {{A, sizeof(double) * B * m * n}, {b, sizeof(double) * B * m},
                           {c, sizeof(double) * B * n},     {extra, sizeof(double) * B * extra_len},
                           {basis, sizeof(int) * B * m},    {run_status, sizeof(int) * B}};   // doubles first
    size_t bytes = 0;
    for (const Part& q : parts) bytes += q.host ? q.bytes : 0;
    LP_HIP(ctx, hipMalloc(&buf.ptr, bytes));
    const void* dev[6] = {};
    hipError_t e = hipSuccess;
    for (size_t i = 0, off = 0; i < 6; ++i) {
        if (!parts[i].host) continue;
        dev[i] = buf.ptr + off;
        if (e == hipSuccess) e = hipMemcpyAsync(buf.ptr + off, parts[i].host, parts[i].bytes, hipMemcpyHostToDevice,
                                                ctx->stream);
        off += parts[i].bytes;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string(what) + " upload: " + hipGetErrorString(e));
    if (A) in.A = static_cast<const double*>(dev[0]);
    if (b) in.b = static_cast<const double*>(dev[1]);
    if (c) in.c = static_cast<const double*>(dev[2]);
    if (extra) in.extra = static_cast<const double*>(dev[3]);
    if (basis) in.basis = static_cast<const int*>(dev[4]);
    if (run_status) in.run_status = static_cast<const int*>(dev[5]);
    return LP_OPTIMAL;
}

// The inputs of a batch handle after its run.  A resident handle's A, b, c, final bases and run statuses are where
// the run left them, and only `extra` goes up.  Any other handle uploads its kept inputs, each LP's final basis and
// the run statuses with it: the same route as a batch of its shape from the host.
static int batch_inputs(lp_batched_problem* p, const char* what, lp_device_buffer& buf, const double* extra,
                        size_t extra_len, BasisInputs& in) {
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const int batch = p->batch, m = p->m, n = p->n;
    if (p->resident) {
        in.A = p->dA;
        in.b = p->db;
        in.c = p->dc;
        in.basis = p->dbasis_out;
        in.run_status = p->dstatus;
        if (!extra) return LP_OPTIMAL;
        return upload(ctx, what, buf, batch, m, n, nullptr, nullptr, nullptr, extra, extra_len, nullptr, nullptr, in);
    }
    return upload(ctx, what, buf, batch, m, n, p->h_A.data(), p->h_b.data(), p->h_c.data(), extra, extra_len,
                  p->h_basis.data(), p->status.data(), in);
}

// Basis checks on the host: LP_BAD_ARG for an index outside [0, n), else LP_OPTIMAL.
static int basis_in_range(const int* basis, int m, int n) {
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) return LP_BAD_ARG;
    return LP_OPTIMAL;
}

// The certificates' basis check: LP_BAD_ARG (an index outside [0, n+m)), LP_SINGULAR (a repeat), else LP_OPTIMAL.
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

static bool run_optimal(int st) { return st == LP_OPTIMAL; }
static bool run_failed(int st) { return st == LP_INFEASIBLE || st == LP_UNBOUNDED; }
static bool wrote_optimal(int rc) { return rc == LP_OPTIMAL; }

// The per-LP path beyond a kernel's fit.  The bases and run statuses come to the host (`basis`).  LP k is taken
// when it has no run status or `eligible` accepts it, and goes through `run(k)` (its lp_basis_X_device call) when
// `check` passes its basis; a failed check, or a return code other than LP_OPTIMAL, becomes its status.  done[k]:
// `written` accepts LP k's return code (its outputs were written).  The statuses go to dstatus.
static int per_lp(lp_context* ctx, int batch, int m, int n, const BasisInputs& in, int* dstatus,
                  bool (*eligible)(int), int (*check)(const int*, int, int), const std::function<int(size_t)>& run,
                  bool (*written)(int), std::vector<char>& done, std::vector<int>& basis) {
    const size_t B = (size_t)batch;
    std::vector<int> st(B, LP_OPTIMAL);
    basis.resize(B * m);
    done.assign(B, 0);
    const int rc = lp_download(ctx, "per-LP path", {{basis.data(), in.basis, sizeof(int) * B * m},
                                                     {st.data(), in.run_status, in.run_status ? sizeof(int) * B : 0}});
    if (rc) return rc;
    for (size_t k = 0; k < B; ++k) {
        if (in.run_status && !eligible(st[k])) continue;
        int cs = check(basis.data() + k * m, m, n);
        if (cs == LP_OPTIMAL) {
            cs = run(k);
            if (cs < 0) return cs;
            done[k] = written(cs);
        }
        if (cs != LP_OPTIMAL) st[k] = cs;
    }
    LP_HIP(ctx, hipMemcpyAsync(dstatus, st.data(), sizeof(int) * B, hipMemcpyHostToDevice, ctx->stream));
    LP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LP_OPTIMAL;
}

extern "C" {

// ===========================================================================
// the dual solution at a given basis (basis_duals.hip)
// ===========================================================================

int lp_basis_duals_fits(int m) { return m > 0 && lp_basis_duals_lds_bytes(m) <= 160 * 1024 ? 1 : 0; }


// Duals of `batch` LPs whose inputs are on the device: LPs whose run status is not LP_OPTIMAL keep it and get NaN.
static int duals_on_device(lp_context* ctx, int batch, int m, int n, const BasisInputs& in, double* y_out,
                           double* d_out, double* w_out, int* status_out) {
    const size_t B = (size_t)batch;
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * B * ((size_t)m + n + 1) + sizeof(int) * B));
    BasisDualsDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.A = in.A;
    d.b = in.b;
    d.c = in.c;
    d.basis = in.basis;
    d.run_status = in.run_status;
    d.y = reinterpret_cast<double*>(buf.ptr);
    d.d = d.y + B * m;
    d.w = d.d + B * n;
    d.status = reinterpret_cast<int*>(d.w + B);
    int rc;
    if (lp_basis_duals_fits(m)) {
        rc = lp_basis_duals_launch(ctx, d);
    } else {
        std::vector<char> done;
        std::vector<int> basis;
        rc = per_lp(ctx, batch, m, n, in, d.status, run_optimal, basis_in_range, [&](size_t k) {
            return lp_basis_duals_device(ctx, in.A + k * m * n, m, n, in.b + k * m, in.c + k * n, in.basis + k * m,
                                         d.y + k * m, d.d + k * n, d.w + k);
        }, wrote_optimal, done, basis);
    }
    if (rc == LP_OPTIMAL)
        rc = lp_download(ctx, "basis duals", {{y_out, d.y, sizeof(double) * B * m},
                                              {d_out, d.d, sizeof(double) * B * n},
                                              {w_out, d.w, sizeof(double) * B},
                                              {status_out, d.status, sizeof(int) * B}});
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

int lp_basis_duals(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                   const int* basis, double* y_out, double* d_out, double* w_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !y_out || !d_out || !w_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_duals: null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_duals: bad dimensions");
    if (basis_in_range(basis, m, n)) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    lp_device_buffer buf;
    BasisInputs in;
    int status = LP_OPTIMAL;
    int rc = upload(ctx, "basis duals", buf, 1, m, n, A, b, c, nullptr, 0, basis, nullptr, in);
    if (rc == LP_OPTIMAL) rc = duals_on_device(ctx, 1, m, n, in, y_out, d_out, w_out, &status);
    return rc ? rc : status;
}

int lp_basis_duals_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                           const double* c, const int* basis, double* y_out, double* d_out, double* w_out,
                           int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !y_out || !d_out || !w_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_duals_batched: null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_duals_batched: bad dimensions");
    lp_device_buffer buf;
    BasisInputs in;
    const int rc = upload(ctx, "basis duals", buf, batch, m, n, A, b, c, nullptr, 0, basis, nullptr, in);
    return rc ? rc : duals_on_device(ctx, batch, m, n, in, y_out, d_out, w_out, status_out);
}

int lp_batched_duals(lp_batched_problem* p, double* y_out, double* d_out, double* w_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!y_out || !d_out || !w_out || !status_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_duals: null argument");
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_duals: the batch has not run");
    lp_device_buffer buf;
    BasisInputs in;
    const int rc = batch_inputs(p, "basis duals", buf, nullptr, 0, in);
    return rc ? rc : duals_on_device(ctx, p->batch, p->m, p->n, in, y_out, d_out, w_out, status_out);
}

// ===========================================================================
// RHS and cost ranging at a given basis (basis_ranging.hip)
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

// Ranges of `batch` LPs whose inputs are on the device: LPs whose run status is not LP_OPTIMAL keep it and get NaN.
static int ranging_on_device(lp_context* ctx, int batch, int m, int n, const BasisInputs& in, int maximize,
                             double eps, double* rhs_out, int* rhs_var_out, double* cost_out, int* cost_var_out,
                             int* status_out) {
    const size_t B = (size_t)batch, nr = B * 2 * m, nc = B * 2 * n;
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * (nr + nc) + sizeof(int) * (nr + nc + B)));
    BasisRangingDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.maximize = maximize ? 1 : 0;
    d.eps = eps;
    d.A = in.A;
    d.b = in.b;
    d.c = in.c;
    d.basis = in.basis;
    d.run_status = in.run_status;
    d.rhs = reinterpret_cast<double*>(buf.ptr);
    d.cost = d.rhs + nr;
    d.rhs_var = reinterpret_cast<int*>(d.cost + nc);
    d.cost_var = d.rhs_var + nr;
    d.status = d.cost_var + nc;
    int rc;
    if (lp_basis_ranging_fits(m, n)) {
        rc = lp_basis_ranging_launch(ctx, d);
    } else {
        std::vector<char> done;
        std::vector<int> basis;
        rc = per_lp(ctx, batch, m, n, in, d.status, run_optimal, basis_in_range, [&](size_t k) {
            return lp_basis_ranging_device(ctx, in.A + k * m * n, m, n, in.b + k * m, in.c + k * n, in.basis + k * m,
                                           d.maximize, eps, d.rhs + k * 2 * m, d.rhs_var + k * 2 * m,
                                           d.cost + k * 2 * n, d.cost_var + k * 2 * n);
        }, wrote_optimal, done, basis);
    }
    if (rc == LP_OPTIMAL)
        rc = lp_download(ctx, "basis ranging", {{rhs_out, d.rhs, sizeof(double) * nr},
                                                {rhs_var_out, d.rhs_var, sizeof(int) * nr},
                                                {cost_out, d.cost, sizeof(double) * nc},
                                                {cost_var_out, d.cost_var, sizeof(int) * nc},
                                                {status_out, d.status, sizeof(int) * B}});
    if (rc != LP_OPTIMAL) return rc;
    // LPs without ranges: NaN (the per-LP path leaves their outputs unwritten)
    for (size_t k = 0; k < B; ++k)
        if (status_out[k] != LP_OPTIMAL) ranging_nan(k, m, n, rhs_out, rhs_var_out, cost_out, cost_var_out);
    return LP_OPTIMAL;
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
    if (basis_in_range(basis, m, n)) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    lp_device_buffer buf;
    BasisInputs in;
    int status = LP_OPTIMAL;
    int rc = upload(ctx, "basis ranging", buf, 1, m, n, A, b, c, nullptr, 0, basis, nullptr, in);
    if (rc == LP_OPTIMAL)
        rc = ranging_on_device(ctx, 1, m, n, in, maximize, eps, rhs_out, rhs_var_out, cost_out, cost_var_out, &status);
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
    lp_device_buffer buf;
    BasisInputs in;
    const int rc = upload(ctx, "basis ranging", buf, batch, m, n, A, b, c, nullptr, 0, basis, nullptr, in);
    return rc ? rc
              : ranging_on_device(ctx, batch, m, n, in, maximize, eps, rhs_out, rhs_var_out, cost_out, cost_var_out,
                                  status_out);
}

int lp_batched_ranging(lp_batched_problem* p, double eps, double* rhs_out, int* rhs_var_out, double* cost_out,
                       int* cost_var_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!rhs_out || !rhs_var_out || !cost_out || !cost_var_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_ranging: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_ranging: eps must be >= 0");
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_ranging: the batch has not run");
    lp_device_buffer buf;
    BasisInputs in;
    const int rc = batch_inputs(p, "basis ranging", buf, nullptr, 0, in);
    return rc ? rc
              : ranging_on_device(ctx, p->batch, p->m, p->n, in, p->maximize, eps, rhs_out, rhs_var_out, cost_out,
                                  cost_var_out, status_out);
}

// ===========================================================================
// The dual solution and ranging of a bounded-variable LP at a given basis and flags (basis_bounded.hip): one LP per
// workgroup for lp_basis_bounded_fits shapes; as in the bounded family there is no handle and no per-LP path for a
// batch.  The _large entries run one LP of any shape on the tableau in HBM.
// ===========================================================================

int lp_basis_bounded_fits(int m, int n) { return lp_basis_bounded_fits_shape(m, n) ? 1 : 0; }

// The checks of lp_simplex_bounded_resolve on every LP of the batch (the pointers and dimensions are the caller's):
// lo finite, hi not NaN, flags 0 or 1 and 1 only under a finite hi, basis indices in [0, n), or in [0, n + m) for the
// certificates (`artificials`): bounded_basis_values; bounded_basis_args adds the fit of the analysis's kernel.
static int bounded_basis_values(lp_context* ctx, const char* who, int batch, int m, int n, const double* lo,
                                const double* hi, const int* basis, const int* at_upper, bool artificials) {
    const size_t N = (size_t)batch * n;
    for (size_t j = 0; j < N; ++j) {
        if (!std::isfinite(lo[j])) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": lo must be finite");
        if (std::isnan(hi[j])) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": hi is NaN");
        if (at_upper[j] != 0 && at_upper[j] != 1) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": at_upper must be 0 or 1");
        if (at_upper[j] && hi[j] == INFINITY)   // (hi = -inf is a crossed bound: that LP's LP_INFEASIBLE)
            LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": a column without an upper bound is flagged at_upper");
    }
    if (basis_in_range(basis, batch * m, artificials ? n + m : n))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": basis index out of range");
    return LP_OPTIMAL;
}

static int bounded_basis_args(lp_context* ctx, const char* who, int batch, int m, int n, const double* lo,
                              const double* hi, const int* basis, const int* at_upper, bool artificials = false) {
    const int rc = bounded_basis_values(ctx, who, batch, m, n, lo, hi, basis, at_upper, artificials);
    if (rc) return rc;
    if (artificials ? !lp_basis_bounded_certificate_fits_shape(m, n) : !lp_basis_bounded_fits_shape(m, n))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the shape does not fit one CU's LDS (lp_basis_bounded" +
                                     (artificials ? "_certificate" : "") + "_fits)");
    return LP_OPTIMAL;
}

// NaN for LP k of the duals outputs
static void bounded_duals_nan(size_t k, int m, int n, double* x, double* y, double* d, double* w) {
    for (size_t j = 0; j < (size_t)n; ++j) x[k * n + j] = d[k * n + j] = NAN;
    for (size_t t = 0; t < (size_t)m; ++t) y[k * m + t] = NAN;
    w[k] = NAN;
}

// NaN values, -1 indices and sides for LP k of the ranging outputs
static void bounded_ranging_nan(size_t k, int m, int n, double* rhs, int* rhs_var, int* rhs_side, double* cost,
                                int* cost_var) {
    ranging_nan(k, m, n, rhs, rhs_var, cost, cost_var);
    for (size_t q = 0; q < 2 * (size_t)m; ++q) rhs_side[k * 2 * m + q] = -1;
}

// The host arrays of `batch` bounded LPs with their bases and flags, and the output arrays of the two analyses.
struct BoundedSensIn {
    int batch, m, n;
    const double *A, *b, *c, *lo, *hi;
    const int *basis, *at_upper;
};
struct BoundedDualsOut {
    double *x, *y, *d, *w;
};
struct BoundedRangingOut {
    double* rhs;
    int *rhs_var, *rhs_side;
    double* cost;
    int* cost_var;
};

// One allocation for the inputs and the outputs of the batch, one launch of k_batched_bounded_sens, one download:
// the ranging launch when `ro` is given (maximize and eps are its), else the duals launch into `du`.  `large` (one LP):
// lp_basis_bounded_device instead of the launch; it returns the LP's status, and nothing comes down unless that is
// LP_OPTIMAL.
static int bounded_sens(lp_context* ctx, const BoundedSensIn& in, const BoundedDualsOut* du, const BoundedRangingOut* ro,
                        int maximize, double eps, int* status_out, bool large = false) {
    const bool ranging = ro != nullptr;
    const int batch = in.batch, m = in.m, n = in.n;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, nr = B * 2 * m, nc = B * 2 * n;
    const size_t in_d = B * ((size_t)m * n + m + 3 * (size_t)n), in_i = B * ((size_t)m + n);
    const size_t out_d = ranging ? nr + nc : B * (2 * (size_t)n + m + 1), out_i = (ranging ? 2 * nr + nc : 0) + B;
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * (in_d + out_d) + sizeof(int) * (in_i + out_i)));
    double* dA = reinterpret_cast<double*>(buf.ptr);   // the doubles first
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    double* dlo = dc + B * n;
    double* dhi = dlo + B * n;
    double* dout = dhi + B * n;
    int* dbasis = reinterpret_cast<int*>(dout + out_d);
    int* dup = dbasis + B * m;
    int* iout = dup + B * n;
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, in.A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, in.b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, in.c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dlo, in.lo, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dhi, in.hi, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, in.basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dup, in.at_upper, sizeof(int) * B * n, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("bounded basis analysis upload: ") + hipGetErrorString(e));
    BasisBoundedDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.maximize = maximize ? 1 : 0;
    d.eps = eps;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.lo = dlo;
    d.hi = dhi;
    d.basis = dbasis;
    d.at_upper = dup;
    int rc;
    if (ranging) {
        d.rhs = dout;
        d.cost = d.rhs + nr;
        d.rhs_var = iout;
        d.rhs_side = d.rhs_var + nr;
        d.cost_var = d.rhs_side + nr;
        d.status = d.cost_var + nc;
        rc = large ? lp_basis_bounded_device(ctx, d, true) : lp_basis_bounded_launch(ctx, d, true);
        if (rc == LP_OPTIMAL)
            rc = lp_download(ctx, "bounded basis ranging", {{ro->rhs, d.rhs, sizeof(double) * nr},
                                                            {ro->cost, d.cost, sizeof(double) * nc},
                                                            {ro->rhs_var, d.rhs_var, sizeof(int) * nr},
                                                            {ro->rhs_side, d.rhs_side, sizeof(int) * nr},
                                                            {ro->cost_var, d.cost_var, sizeof(int) * nc},
                                                            {status_out, d.status, large ? 0 : sizeof(int) * B}});
    } else {
        d.x = dout;
        d.d = d.x + B * n;
        d.y = d.d + B * n;
        d.w = d.y + B * m;
        d.status = iout;
        rc = large ? lp_basis_bounded_device(ctx, d, false) : lp_basis_bounded_launch(ctx, d, false);
        if (rc == LP_OPTIMAL)
            rc = lp_download(ctx, "bounded basis duals", {{du->x, d.x, sizeof(double) * B * n},
                                                          {du->d, d.d, sizeof(double) * B * n},
                                                          {du->y, d.y, sizeof(double) * B * m},
                                                          {du->w, d.w, sizeof(double) * B},
                                                          {status_out, d.status, large ? 0 : sizeof(int) * B}});
    }
    return rc;
}

// lp_basis_bounded_duals (`who`), or with `large` lp_basis_bounded_duals_large: the same checks without the fit
static int bounded_duals_one(lp_context* ctx, const char* who, bool large, const double* A, int m, int n,
                             const double* b, const double* c, const double* lo, const double* hi, const int* basis,
                             const int* at_upper, double* x_out, double* y_out, double* d_out, double* w_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !lo || !hi || !basis || !at_upper || !x_out || !y_out || !d_out || !w_out)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    bounded_duals_nan(0, m, n, x_out, y_out, d_out, w_out);
    int rc = large ? bounded_basis_values(ctx, who, 1, m, n, lo, hi, basis, at_upper, false)
                   : bounded_basis_args(ctx, who, 1, m, n, lo, hi, basis, at_upper);
    if (rc) return rc;
    int status = LP_OPTIMAL;
    const BoundedDualsOut out{x_out, y_out, d_out, w_out};
    rc = bounded_sens(ctx, {1, m, n, A, b, c, lo, hi, basis, at_upper}, &out, nullptr, 0, 0.0, &status, large);
    return rc ? rc : status;
}

int lp_basis_bounded_duals(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                           const double* lo, const double* hi, const int* basis, const int* at_upper, double* x_out,
                           double* y_out, double* d_out, double* w_out) {
    return bounded_duals_one(ctx, "lp_basis_bounded_duals", false, A, m, n, b, c, lo, hi, basis, at_upper, x_out,
                             y_out, d_out, w_out);
}

int lp_basis_bounded_duals_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                 const double* lo, const double* hi, const int* basis, const int* at_upper,
                                 double* x_out, double* y_out, double* d_out, double* w_out) {
    return bounded_duals_one(ctx, "lp_basis_bounded_duals_large", true, A, m, n, b, c, lo, hi, basis, at_upper, x_out,
                             y_out, d_out, w_out);
}

int lp_basis_bounded_duals_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                   const double* c, const double* lo, const double* hi, const int* basis,
                                   const int* at_upper, double* x_out, double* y_out, double* d_out, double* w_out,
                                   int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !lo || !hi || !basis || !at_upper || !x_out || !y_out || !d_out || !w_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_bounded_duals_batched: null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_bounded_duals_batched: bad dimensions");
    const int rc = bounded_basis_args(ctx, "lp_basis_bounded_duals_batched", batch, m, n, lo, hi, basis, at_upper);
    if (rc) return rc;
    const BoundedDualsOut out{x_out, y_out, d_out, w_out};
    return bounded_sens(ctx, {batch, m, n, A, b, c, lo, hi, basis, at_upper}, &out, nullptr, 0, 0.0, status_out);
}

// lp_basis_bounded_ranging (`who`), or with `large` lp_basis_bounded_ranging_large: the same checks without the fit
static int bounded_ranging_one(lp_context* ctx, const char* who, bool large, const double* A, int m, int n,
                               const double* b, const double* c, const double* lo, const double* hi, const int* basis,
                               const int* at_upper, int maximize, double eps, double* rhs_out, int* rhs_var_out,
                               int* rhs_side_out, double* cost_out, int* cost_var_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !lo || !hi || !basis || !at_upper || !rhs_out || !rhs_var_out || !rhs_side_out ||
        !cost_out || !cost_var_out)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    bounded_ranging_nan(0, m, n, rhs_out, rhs_var_out, rhs_side_out, cost_out, cost_var_out);
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": eps must be >= 0");
    int rc = large ? bounded_basis_values(ctx, who, 1, m, n, lo, hi, basis, at_upper, false)
                   : bounded_basis_args(ctx, who, 1, m, n, lo, hi, basis, at_upper);
    if (rc) return rc;
    int status = LP_OPTIMAL;
    const BoundedRangingOut out{rhs_out, rhs_var_out, rhs_side_out, cost_out, cost_var_out};
    rc = bounded_sens(ctx, {1, m, n, A, b, c, lo, hi, basis, at_upper}, nullptr, &out, maximize, eps, &status, large);
    return rc ? rc : status;
}

int lp_basis_bounded_ranging(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                             const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize,
                             double eps, double* rhs_out, int* rhs_var_out, int* rhs_side_out, double* cost_out,
                             int* cost_var_out) {
    return bounded_ranging_one(ctx, "lp_basis_bounded_ranging", false, A, m, n, b, c, lo, hi, basis, at_upper,
                               maximize, eps, rhs_out, rhs_var_out, rhs_side_out, cost_out, cost_var_out);
}

int lp_basis_bounded_ranging_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                   const double* lo, const double* hi, const int* basis, const int* at_upper,
                                   int maximize, double eps, double* rhs_out, int* rhs_var_out, int* rhs_side_out,
                                   double* cost_out, int* cost_var_out) {
    return bounded_ranging_one(ctx, "lp_basis_bounded_ranging_large", true, A, m, n, b, c, lo, hi, basis, at_upper,
                               maximize, eps, rhs_out, rhs_var_out, rhs_side_out, cost_out, cost_var_out);
}

int lp_basis_bounded_ranging_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                     const double* c, const double* lo, const double* hi, const int* basis,
                                     const int* at_upper, int maximize, double eps, double* rhs_out, int* rhs_var_out,
                                     int* rhs_side_out, double* cost_out, int* cost_var_out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !lo || !hi || !basis || !at_upper || !rhs_out || !rhs_var_out || !rhs_side_out ||
        !cost_out || !cost_var_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_bounded_ranging_batched: null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_bounded_ranging_batched: bad dimensions");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_bounded_ranging_batched: eps must be >= 0");
    const int rc = bounded_basis_args(ctx, "lp_basis_bounded_ranging_batched", batch, m, n, lo, hi, basis, at_upper);
    if (rc) return rc;
    const BoundedRangingOut out{rhs_out, rhs_var_out, rhs_side_out, cost_out, cost_var_out};
    return bounded_sens(ctx, {batch, m, n, A, b, c, lo, hi, basis, at_upper}, nullptr, &out, maximize, eps, status_out);
}

// ===========================================================================
// Farkas and unbounded-ray certificates at a given basis (basis_certificate.hip)
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

// Certificates of `batch` LPs whose inputs are on the device: with run statuses, only LPs whose run status is
// LP_INFEASIBLE / LP_UNBOUNDED get one, the others keep it and get NONE.
static int certificate_on_device(lp_context* ctx, int batch, int m, int n, const BasisInputs& in, int maximize,
                                 double eps, int* kind_out, double* farkas_out, double* ray_out, double* value_out,
                                 int* index_out, int* status_out) {
    const size_t B = (size_t)batch, nf = B * m, nr = B * n;
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * (nf + nr + B) + sizeof(int) * 3 * B));
    BasisCertificateDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.maximize = maximize ? 1 : 0;
    d.eps = eps;
    d.A = in.A;
    d.b = in.b;
    d.c = in.c;
    d.basis = in.basis;
    d.run_status = in.run_status;
    d.farkas = reinterpret_cast<double*>(buf.ptr);
    d.ray = d.farkas + nf;
    d.value = d.ray + nr;
    d.kind = reinterpret_cast<int*>(d.value + B);
    d.index = d.kind + B;
    d.status = d.index + B;
    std::vector<char> done(B, 1);   // the LP's outputs were written on the device
    int rc;
    if (lp_basis_certificate_fits(m, n)) {
        rc = lp_basis_certificate_launch(ctx, d);
    } else {
        std::vector<int> basis;
        rc = per_lp(ctx, batch, m, n, in, d.status, run_failed, certificate_basis_check, [&](size_t k) {
            return lp_basis_certificate_device(ctx, in.A + k * m * n, m, n, in.b + k * m, in.c + k * n,
                                               in.basis + k * m, d.maximize, eps, d.kind + k, d.farkas + k * m,
                                               d.ray + k * n, d.value + k, d.index + k);
        }, wrote_optimal, done, basis);
    }
    if (rc == LP_OPTIMAL)
        rc = lp_download(ctx, "basis certificate", {{farkas_out, d.farkas, sizeof(double) * nf},
                                                    {ray_out, d.ray, sizeof(double) * nr},
                                                    {value_out, d.value, sizeof(double) * B},
                                                    {kind_out, d.kind, sizeof(int) * B},
                                                    {index_out, d.index, sizeof(int) * B},
                                                    {status_out, d.status, sizeof(int) * B}});
    if (rc != LP_OPTIMAL) return rc;
    // LPs without a certificate on the per-LP path: NONE (their outputs were left unwritten)
    for (size_t k = 0; k < B; ++k)
        if (!done[k]) certificate_none(k, m, n, kind_out, farkas_out, ray_out, value_out, index_out);
    return LP_OPTIMAL;
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
    lp_device_buffer buf;
    BasisInputs in;
    int status = LP_OPTIMAL;
    int rc = upload(ctx, "basis certificate", buf, 1, m, n, A, b, c, nullptr, 0, basis, nullptr, in);
    if (rc == LP_OPTIMAL)
        rc = certificate_on_device(ctx, 1, m, n, in, maximize, eps, kind_out, farkas_out, ray_out, value_out,
                                   index_out, &status);
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
    lp_device_buffer buf;
    BasisInputs in;
    const int rc = upload(ctx, "basis certificate", buf, batch, m, n, A, b, c, nullptr, 0, basis, nullptr, in);
    return rc ? rc
              : certificate_on_device(ctx, batch, m, n, in, maximize, eps, kind_out, farkas_out, ray_out, value_out,
                                      index_out, status_out);
}

int lp_batched_certificates(lp_batched_problem* p, double eps, int* kind_out, double* farkas_out, double* ray_out,
                            double* value_out, int* index_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!kind_out || !farkas_out || !ray_out || !value_out || !index_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_certificates: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_certificates: eps must be >= 0");
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_certificates: the batch has not run");
    lp_device_buffer buf;
    BasisInputs in;
    const int rc = batch_inputs(p, "basis certificate", buf, nullptr, 0, in);
    return rc ? rc
              : certificate_on_device(ctx, p->batch, p->m, p->n, in, p->maximize, eps, kind_out, farkas_out, ray_out,
                                      value_out, index_out, status_out);
}

// ===========================================================================
// Farkas and unbounded-ray certificates of a bounded-variable LP at a given basis and flags
// (basis_bounded_certificate.hip): one LP per workgroup for lp_basis_bounded_certificate_fits shapes;
// lp_basis_bounded_certificate_large runs one LP of any shape on the tableau in HBM
// ===========================================================================

int lp_basis_bounded_certificate_fits(int m, int n) { return lp_basis_bounded_certificate_fits_shape(m, n) ? 1 : 0; }

struct BoundedCertificateOut {
    int* kind;
    double *farkas, *ray, *value;
    int* index;
};

// One allocation for the inputs and the outputs of the batch, uploads queued on the context's stream, one launch of
// k_batched_bounded_certificate, one download.  run_status may be nullptr.  `large` (one LP, no run_status):
// lp_basis_bounded_certificate_device instead of the launch; it returns the LP's status, and nothing comes down unless
// that is LP_OPTIMAL.
static int bounded_certificate(lp_context* ctx, const BoundedSensIn& in, const int* run_status, int maximize, double eps,
                               const BoundedCertificateOut& out, int* status_out, bool large = false) {
    const int batch = in.batch, m = in.m, n = in.n;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, nf = B * m, nr = B * n;
    const size_t in_d = B * ((size_t)m * n + m + 3 * (size_t)n), in_i = B * ((size_t)m + n + (run_status ? 1 : 0));
    const size_t out_d = nf + nr + B, out_i = 3 * B;
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * (in_d + out_d) + sizeof(int) * (in_i + out_i)));
    double* dA = reinterpret_cast<double*>(buf.ptr);   // the doubles first
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    double* dlo = dc + B * n;
    double* dhi = dlo + B * n;
    double* dout = dhi + B * n;
    int* dbasis = reinterpret_cast<int*>(dout + out_d);
    int* dup = dbasis + B * m;
    int* drun = dup + B * n;
    int* iout = drun + (run_status ? B : 0);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, in.A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, in.b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, in.c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dlo, in.lo, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dhi, in.hi, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, in.basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dup, in.at_upper, sizeof(int) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && run_status) e = hipMemcpyAsync(drun, run_status, sizeof(int) * B, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("bounded basis certificate upload: ") + hipGetErrorString(e));
    BasisBoundedCertificateDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.maximize = maximize ? 1 : 0;
    d.eps = eps;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.lo = dlo;
    d.hi = dhi;
    d.basis = dbasis;
    d.at_upper = dup;
    d.run_status = run_status ? drun : nullptr;
    d.farkas = dout;
    d.ray = d.farkas + nf;
    d.value = d.ray + nr;
    d.kind = iout;
    d.index = d.kind + B;
    d.status = d.index + B;
    int rc = large ? lp_basis_bounded_certificate_device(ctx, d) : lp_basis_bounded_certificate_launch(ctx, d);
    if (rc == LP_OPTIMAL)
        rc = lp_download(ctx, "bounded basis certificate", {{out.farkas, d.farkas, sizeof(double) * nf},
                                                            {out.ray, d.ray, sizeof(double) * nr},
                                                            {out.value, d.value, sizeof(double) * B},
                                                            {out.kind, d.kind, sizeof(int) * B},
                                                            {out.index, d.index, sizeof(int) * B},
                                                            {status_out, d.status, large ? 0 : sizeof(int) * B}});
    return rc;
}

// lp_basis_bounded_certificate (`who`), or with `large` lp_basis_bounded_certificate_large: the same checks without
// the fit.  The kernel looks for a repeated index itself; the single-LP device path leaves that to the host, which
// answers as the definition orders it: crossed bounds (LP_INFEASIBLE) before a repeat (LP_SINGULAR).
static int bounded_certificate_one(lp_context* ctx, const char* who, bool large, const double* A, int m, int n,
                                   const double* b, const double* c, const double* lo, const double* hi,
                                   const int* basis, const int* at_upper, int maximize, double eps, int* kind_out,
                                   double* farkas_out, double* ray_out, double* value_out, int* index_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !lo || !hi || !basis || !at_upper || !kind_out || !farkas_out || !ray_out || !value_out ||
        !index_out)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    certificate_none(0, m, n, kind_out, farkas_out, ray_out, value_out, index_out);
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": eps must be >= 0");
    int rc = large ? bounded_basis_values(ctx, who, 1, m, n, lo, hi, basis, at_upper, true)
                   : bounded_basis_args(ctx, who, 1, m, n, lo, hi, basis, at_upper, true);
    if (rc) return rc;
    if (large && certificate_basis_check(basis, m, n) == LP_SINGULAR) {
        for (int j = 0; j < n; ++j)
            if (hi[j] < lo[j]) return LP_INFEASIBLE;
        return LP_SINGULAR;
    }
    int status = LP_OPTIMAL;
    rc = bounded_certificate(ctx, {1, m, n, A, b, c, lo, hi, basis, at_upper}, nullptr, maximize, eps,
                             {kind_out, farkas_out, ray_out, value_out, index_out}, &status, large);
    return rc ? rc : status;
}

int lp_basis_bounded_certificate(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                 const double* lo, const double* hi, const int* basis, const int* at_upper,
                                 int maximize, double eps, int* kind_out, double* farkas_out, double* ray_out,
                                 double* value_out, int* index_out) {
    return bounded_certificate_one(ctx, "lp_basis_bounded_certificate", false, A, m, n, b, c, lo, hi, basis, at_upper,
                                   maximize, eps, kind_out, farkas_out, ray_out, value_out, index_out);
}

int lp_basis_bounded_certificate_large(lp_context* ctx, const double* A, int m, int n, const double* b,
                                       const double* c, const double* lo, const double* hi, const int* basis,
                                       const int* at_upper, int maximize, double eps, int* kind_out,
                                       double* farkas_out, double* ray_out, double* value_out, int* index_out) {
    return bounded_certificate_one(ctx, "lp_basis_bounded_certificate_large", true, A, m, n, b, c, lo, hi, basis,
                                   at_upper, maximize, eps, kind_out, farkas_out, ray_out, value_out, index_out);
}

int lp_basis_bounded_certificate_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                         const double* c, const double* lo, const double* hi, const int* basis,
                                         const int* at_upper, const int* run_status, int maximize, double eps,
                                         int* kind_out, double* farkas_out, double* ray_out, double* value_out,
                                         int* index_out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !lo || !hi || !basis || !at_upper || !kind_out || !farkas_out || !ray_out || !value_out ||
        !index_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_bounded_certificate_batched: null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_bounded_certificate_batched: bad dimensions");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_basis_bounded_certificate_batched: eps must be >= 0");
    const int rc = bounded_basis_args(ctx, "lp_basis_bounded_certificate_batched", batch, m, n, lo, hi, basis, at_upper,
                                      true);
    if (rc) return rc;
    return bounded_certificate(ctx, {batch, m, n, A, b, c, lo, hi, basis, at_upper}, run_status, maximize, eps,
                               {kind_out, farkas_out, ray_out, value_out, index_out}, status_out);
}

// ===========================================================================
// Parametric right-hand side and parametric cost from an optimal basis (basis_parametric.hip,
// basis_parametric_cost.hip)
// ===========================================================================

int lp_basis_parametric_fits(int m, int n) {
    return m > 0 && n >= m && lp_basis_parametric_lds_bytes(m, n, nullptr) <= 160 * 1024 ? 1 : 0;
}

int lp_basis_parametric_cost_fits(int m, int n) {
    return m > 0 && n >= m && lp_basis_parametric_cost_lds_bytes(m, n, nullptr) <= 160 * 1024 ? 1 : 0;
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

// After the per-LP path (basis: the given bases), which writes the path only: the rest is NaN / -1, and LPs without
// one get it all.
static void parametric_pad(size_t B, int m, int mb, const std::vector<char>& done, const std::vector<int>& basis,
                           int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                           int* leave_out, int* basis_out) {
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
}

// The argument checks shared by the entry points of both parametric analyses (LP_OPTIMAL when they pass)
static int parametric_args(lp_context* ctx, const char* fn, double t_max, double eps, int max_breaks) {
    if (max_breaks < 0) LP_FAIL(ctx, LP_BAD_ARG, std::string(fn) + ": max_breaks must be >= 0");
    if (!(t_max >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(fn) + ": t_max must be >= 0");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(fn) + ": eps must be >= 0");
    return LP_OPTIMAL;
}

// The statuses with which the per-LP path has written a path: the right-hand side's ends infeasible, the cost's unbounded
static bool rhs_path_written(int st) { return st == LP_OPTIMAL || st == LP_INFEASIBLE || st == LP_ITER_LIMIT; }
static bool cost_path_written(int st) { return st == LP_OPTIMAL || st == LP_UNBOUNDED || st == LP_ITER_LIMIT; }

struct ParametricOut {
    int* nseg;
    double *t, *obj, *slope;
    int *enter, *leave, *basis;
};

// Paths of `batch` LPs whose inputs (the direction in in.extra: d, m per LP, or with `cost` g, n per LP) are on the
// device: LPs whose run status is not LP_OPTIMAL keep it and get nseg 0.
static int parametric_on_device(lp_context* ctx, int batch, int m, int n, const BasisInputs& in, bool cost,
                                int maximize, double t_max, double eps, int mb, const ParametricOut& out,
                                int* status_out) {
    const size_t B = (size_t)batch, nt = B * (mb + 2), ns = B * (mb + 1), nd = cost ? n : m;
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * (2 * nt + ns) + sizeof(int) * (2 * ns + B * m + 2 * B)));
    BasisParametricDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    (void)(cost ? lp_basis_parametric_cost_lds_bytes : lp_basis_parametric_lds_bytes)(m, n, &d.pitch);
    d.max_breaks = mb;
    d.eps = eps;
    d.t_max = t_max;
    d.A = in.A;
    d.b = in.b;
    d.c = in.c;
    d.dir = in.extra;
    d.basis = in.basis;
    d.run_status = in.run_status;
    d.t = reinterpret_cast<double*>(buf.ptr);
    d.obj = d.t + nt;
    d.slope = d.obj + nt;
    d.enter = reinterpret_cast<int*>(d.slope + ns);
    d.leave = d.enter + ns;
    d.basis_out = d.leave + ns;
    d.nseg = d.basis_out + B * m;
    d.status = d.nseg + B;
    std::vector<char> done;
    std::vector<int> basis;   // per-LP path: the given bases
    int rc;
    if ((cost ? lp_basis_parametric_cost_fits : lp_basis_parametric_fits)(m, n)) {
        rc = (cost ? lp_basis_parametric_cost_launch : lp_basis_parametric_launch)(ctx, d, maximize);
    } else {
        const auto device = cost ? lp_basis_parametric_cost_device : lp_basis_parametric_device;
        rc = per_lp(ctx, batch, m, n, in, d.status, run_optimal, basis_in_range, [&](size_t k) {
            return device(ctx, in.A + k * m * n, m, n, in.b + k * m, in.c + k * n, in.basis + k * m,
                          in.extra + k * nd, maximize, t_max, eps, mb, d.nseg + k, d.t + k * (mb + 2),
                          d.obj + k * (mb + 2), d.slope + k * (mb + 1), d.enter + k * (mb + 1),
                          d.leave + k * (mb + 1), d.basis_out + k * m);
        }, cost ? cost_path_written : rhs_path_written, done, basis);
    }
    if (rc == LP_OPTIMAL)
        rc = lp_download(ctx, cost ? "basis parametric cost" : "basis parametric",
                         {{out.t, d.t, sizeof(double) * nt},
                          {out.obj, d.obj, sizeof(double) * nt},
                          {out.slope, d.slope, sizeof(double) * ns},
                          {out.enter, d.enter, sizeof(int) * ns},
                          {out.leave, d.leave, sizeof(int) * ns},
                          {out.basis, d.basis_out, sizeof(int) * B * m},
                          {out.nseg, d.nseg, sizeof(int) * B},
                          {status_out, d.status, sizeof(int) * B}});
    if (rc != LP_OPTIMAL) return rc;
    if (!basis.empty())
        parametric_pad(B, m, mb, done, basis, out.nseg, out.t, out.obj, out.slope, out.enter, out.leave, out.basis);
    return LP_OPTIMAL;
}

static bool parametric_out_null(const ParametricOut& o) {
    return !o.nseg || !o.t || !o.obj || !o.slope || !o.enter || !o.leave || !o.basis;
}

// The single-LP entry of either path
static int parametric_one(lp_context* ctx, const char* who, bool cost, const double* A, int m, int n, const double* b,
                          const double* c, const int* basis, int maximize, const double* dir, double t_max, double eps,
                          int max_breaks, const ParametricOut& out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !dir || parametric_out_null(out))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    if (max_breaks < 0) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": max_breaks must be >= 0");
    parametric_none(0, m, max_breaks, basis, out.nseg, out.t, out.obj, out.slope, out.enter, out.leave, out.basis);
    int rc = parametric_args(ctx, who, t_max, eps, max_breaks);
    if (rc) return rc;
    if (basis_in_range(basis, m, n)) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    lp_device_buffer buf;
    BasisInputs in;
    int status = LP_OPTIMAL;
    rc = upload(ctx, cost ? "basis parametric cost" : "basis parametric", buf, 1, m, n, A, b, c, dir,
                (size_t)(cost ? n : m), basis, nullptr, in);
    if (rc == LP_OPTIMAL)
        rc = parametric_on_device(ctx, 1, m, n, in, cost, maximize, t_max, eps, max_breaks, out, &status);
    if (rc) return rc;
    if (status == LP_BAD_ARG) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the basis is not optimal at t = 0");
    return status;
}

// The batched entry of either path
static int parametric_many(lp_context* ctx, const char* who, bool cost, int batch, const double* A, int m, int n,
                           const double* b, const double* c, const int* basis, int maximize, const double* dir,
                           double t_max, double eps, int max_breaks, const ParametricOut& out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !basis || !dir || parametric_out_null(out) || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    int rc = parametric_args(ctx, who, t_max, eps, max_breaks);
    if (rc) return rc;
    lp_device_buffer buf;
    BasisInputs in;
    rc = upload(ctx, cost ? "basis parametric cost" : "basis parametric", buf, batch, m, n, A, b, c, dir,
                (size_t)(cost ? n : m), basis, nullptr, in);
    return rc ? rc
              : parametric_on_device(ctx, batch, m, n, in, cost, maximize, t_max, eps, max_breaks, out, status_out);
}

// The entry of either path on a batch handle that has run
static int parametric_handle(lp_batched_problem* p, const char* who, bool cost, const double* dir, double t_max,
                             double eps, int max_breaks, const ParametricOut& out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!dir || parametric_out_null(out) || !status_out) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    int rc = parametric_args(ctx, who, t_max, eps, max_breaks);
    if (rc) return rc;
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the batch has not run");
    lp_device_buffer buf;
    BasisInputs in;
    rc = batch_inputs(p, cost ? "basis parametric cost" : "basis parametric", buf, dir, (size_t)(cost ? p->n : p->m),
                      in);
    return rc ? rc
              : parametric_on_device(ctx, p->batch, p->m, p->n, in, cost, p->maximize, t_max, eps, max_breaks, out,
                                     status_out);
}

int lp_basis_parametric(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                        const int* basis, int maximize, const double* d, double t_max, double eps, int max_breaks,
                        int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                        int* leave_out, int* basis_out) {
    return parametric_one(ctx, "lp_basis_parametric", false, A, m, n, b, c, basis, maximize, d, t_max, eps, max_breaks,
                          {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out});
}

int lp_basis_parametric_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                const double* c, const int* basis, int maximize, const double* d, double t_max,
                                double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out,
                                double* slope_out, int* enter_out, int* leave_out, int* basis_out, int* status_out) {
    return parametric_many(ctx, "lp_basis_parametric_batched", false, batch, A, m, n, b, c, basis, maximize, d, t_max,
                           eps, max_breaks, {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out},
                           status_out);
}

int lp_batched_parametric(lp_batched_problem* p, const double* d, double t_max, double eps, int max_breaks,
                          int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                          int* leave_out, int* basis_out, int* status_out) {
    return parametric_handle(p, "lp_batched_parametric", false, d, t_max, eps, max_breaks,
                             {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out}, status_out);
}

int lp_basis_parametric_cost(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                             const int* basis, int maximize, const double* g, double t_max, double eps, int max_breaks,
                             int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                             int* leave_out, int* basis_out) {
    return parametric_one(ctx, "lp_basis_parametric_cost", true, A, m, n, b, c, basis, maximize, g, t_max, eps,
                          max_breaks, {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out});
}

int lp_basis_parametric_cost_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                     const double* c, const int* basis, int maximize, const double* g, double t_max,
                                     double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out,
                                     double* slope_out, int* enter_out, int* leave_out, int* basis_out, int* status_out) {
    return parametric_many(ctx, "lp_basis_parametric_cost_batched", true, batch, A, m, n, b, c, basis, maximize, g,
                           t_max, eps, max_breaks,
                           {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out}, status_out);
}

int lp_batched_parametric_cost(lp_batched_problem* p, const double* g, double t_max, double eps, int max_breaks,
                               int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                               int* leave_out, int* basis_out, int* status_out) {
    return parametric_handle(p, "lp_batched_parametric_cost", true, g, t_max, eps, max_breaks,
                             {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, basis_out}, status_out);
}

// ===========================================================================
// Parametric right-hand side and parametric cost of a bounded-variable LP from an optimal basis and its at-upper flags
// (basis_bounded_parametric.hip): one LP per workgroup for lp_basis_bounded_parametric_fits / _cost_fits shapes only;
// as in the bounded family there is no handle and no per-LP path.  The _large entries run one LP of any shape on the
// tableau in HBM (basis_bounded_parametric_large.hip)
// ===========================================================================

int lp_basis_bounded_parametric_fits(int m, int n) { return lp_basis_bounded_parametric_fits_shape(m, n, false) ? 1 : 0; }

int lp_basis_bounded_parametric_cost_fits(int m, int n) {
    return lp_basis_bounded_parametric_fits_shape(m, n, true) ? 1 : 0;
}

struct BoundedParametricOut {
    int* nseg;
    double *t, *obj, *slope;
    int *enter, *leave, *side, *basis, *at_upper;
};

// LP k without a path: parametric_none, side -1 and the given flags (host) back
static void bounded_parametric_none(size_t k, int m, int n, int mb, const int* basis, const int* at_upper,
                                    const BoundedParametricOut& o) {
    parametric_none(k, m, mb, basis, o.nseg, o.t, o.obj, o.slope, o.enter, o.leave, o.basis);
    for (size_t q = 0; q < (size_t)mb + 1; ++q) o.side[k * (mb + 1) + q] = -1;
    std::memcpy(o.at_upper + k * n, at_upper, sizeof(int) * (size_t)n);
}

// The checks every entry point of the two analyses shares after its null and dimension checks: the path's arguments,
// the bounds, flags and indices of every LP, and the fit of the path's kernel
static int bounded_parametric_args(lp_context* ctx, const char* who, const BoundedSensIn& in, bool cost, double t_max,
                                   double eps, int max_breaks) {
    int rc = parametric_args(ctx, who, t_max, eps, max_breaks);
    if (rc) return rc;
    rc = bounded_basis_values(ctx, who, in.batch, in.m, in.n, in.lo, in.hi, in.basis, in.at_upper, false);
    if (rc) return rc;
    if (!lp_basis_bounded_parametric_fits_shape(in.m, in.n, cost))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the shape does not fit one CU's LDS (lp_basis_bounded_parametric" +
                                     (cost ? "_cost" : "") + "_fits)");
    return LP_OPTIMAL;
}

// One allocation for the inputs and the outputs of the batch, uploads queued on the context's stream, one launch of
// k_batched_bounded_parametric or k_batched_bounded_parametric_cost, one download.  `dir` is d (m per LP) or g (n per
// LP); run_status may be nullptr.  `large` (one LP, no run_status, `out` already holding bounded_parametric_none's
// fill): lp_basis_bounded_parametric_device instead of the launch; it returns the LP's status into *status_out, and
// only the path it wrote comes down.
static int bounded_parametric(lp_context* ctx, const BoundedSensIn& in, const double* dir, bool cost,
                              const int* run_status, int maximize, double t_max, double eps, int mb,
                              const BoundedParametricOut& out, int* status_out, bool large = false) {
    const int batch = in.batch, m = in.m, n = in.n;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)batch, nt = B * (mb + 2), ns = B * (mb + 1), nd = B * (cost ? n : m);
    const size_t in_d = B * ((size_t)m * n + m + 3 * (size_t)n) + nd, in_i = B * ((size_t)m + n + (run_status ? 1 : 0));
    const size_t out_d = 2 * nt + ns, out_i = 3 * ns + B * ((size_t)m + n + 2);
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * (in_d + out_d) + sizeof(int) * (in_i + out_i)));
    double* dA = reinterpret_cast<double*>(buf.ptr);   // the doubles first
    double* db = dA + B * m * n;
    double* dc = db + B * m;
    double* dlo = dc + B * n;
    double* dhi = dlo + B * n;
    double* ddir = dhi + B * n;
    double* dout = ddir + nd;
    int* dbasis = reinterpret_cast<int*>(dout + out_d);
    int* dup = dbasis + B * m;
    int* drun = dup + B * n;
    int* iout = drun + (run_status ? B : 0);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(dA, in.A, sizeof(double) * B * m * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(db, in.b, sizeof(double) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, in.c, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dlo, in.lo, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dhi, in.hi, sizeof(double) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ddir, dir, sizeof(double) * nd, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dbasis, in.basis, sizeof(int) * B * m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dup, in.at_upper, sizeof(int) * B * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && run_status) e = hipMemcpyAsync(drun, run_status, sizeof(int) * B, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("bounded basis parametric upload: ") + hipGetErrorString(e));
    BasisBoundedParametricDev d{};
    d.batch = batch;
    d.m = m;
    d.n = n;
    d.maximize = maximize ? 1 : 0;
    d.max_breaks = mb;
    d.eps = eps;
    d.t_max = t_max;
    d.A = dA;
    d.b = db;
    d.c = dc;
    d.lo = dlo;
    d.hi = dhi;
    d.dir = ddir;
    d.basis = dbasis;
    d.at_upper = dup;
    d.run_status = run_status ? drun : nullptr;
    d.t = dout;
    d.obj = d.t + nt;
    d.slope = d.obj + nt;
    d.enter = iout;
    d.leave = d.enter + ns;
    d.side = d.leave + ns;
    d.basis_out = d.side + ns;
    d.at_upper_out = d.basis_out + B * m;
    d.nseg = d.at_upper_out + B * n;
    d.status = d.nseg + B;
    if (large) {
        int nseg = 0;
        const int st = lp_basis_bounded_parametric_device(ctx, d, cost, &nseg);
        if (st < 0) return st;
        *status_out = st;
        if (nseg <= 0) return LP_OPTIMAL;
        const size_t np = (size_t)nseg;
        return lp_download(ctx, "bounded basis parametric", {{out.t, d.t, sizeof(double) * (np + 1)},
                                                             {out.obj, d.obj, sizeof(double) * (np + 1)},
                                                             {out.slope, d.slope, sizeof(double) * np},
                                                             {out.enter, d.enter, sizeof(int) * np},
                                                             {out.leave, d.leave, sizeof(int) * np},
                                                             {out.side, d.side, sizeof(int) * np},
                                                             {out.basis, d.basis_out, sizeof(int) * (size_t)m},
                                                             {out.at_upper, d.at_upper_out, sizeof(int) * (size_t)n},
                                                             {out.nseg, d.nseg, sizeof(int)}});
    }
    int rc = lp_basis_bounded_parametric_launch(ctx, d, cost);
    if (rc == LP_OPTIMAL)
        rc = lp_download(ctx, "bounded basis parametric", {{out.t, d.t, sizeof(double) * nt},
                                                           {out.obj, d.obj, sizeof(double) * nt},
                                                           {out.slope, d.slope, sizeof(double) * ns},
                                                           {out.enter, d.enter, sizeof(int) * ns},
                                                           {out.leave, d.leave, sizeof(int) * ns},
                                                           {out.side, d.side, sizeof(int) * ns},
                                                           {out.basis, d.basis_out, sizeof(int) * B * m},
                                                           {out.at_upper, d.at_upper_out, sizeof(int) * B * n},
                                                           {out.nseg, d.nseg, sizeof(int) * B},
                                                           {status_out, d.status, sizeof(int) * B}});
    return rc;
}

// The single-LP entry of either path (`who`), or with `large` its _large form: the same checks in the same order
// without the fit (the selectors' LDS bounds m instead), and crossed bounds answered here as the definition orders
// them, after every LP_BAD_ARG and before the crash can say LP_SINGULAR
static int bounded_parametric_one(lp_context* ctx, const char* who, bool large, bool cost, const double* A, int m, int n,
                                  const double* b, const double* c, const double* lo, const double* hi,
                                  const int* basis, const int* at_upper, int maximize, const double* dir, double t_max,
                                  double eps, int max_breaks, const BoundedParametricOut& out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !lo || !hi || !basis || !at_upper || !dir || !out.nseg || !out.t || !out.obj || !out.slope ||
        !out.enter || !out.leave || !out.side || !out.basis || !out.at_upper)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    if (max_breaks < 0) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": max_breaks must be >= 0");
    bounded_parametric_none(0, m, n, max_breaks, basis, at_upper, out);
    const BoundedSensIn in{1, m, n, A, b, c, lo, hi, basis, at_upper};
    int rc;
    if (large) {
        rc = parametric_args(ctx, who, t_max, eps, max_breaks);
        if (rc == LP_OPTIMAL) rc = bounded_basis_values(ctx, who, 1, m, n, lo, hi, basis, at_upper, false);
        if (rc) return rc;
        if (lp_basis_bounded_parametric_large_lds_bytes(m, cost) > 156 * 1024)
            LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": m too large for the selector's LDS");
        for (int j = 0; j < n; ++j)
            if (hi[j] < lo[j]) return LP_INFEASIBLE;
    } else {
        rc = bounded_parametric_args(ctx, who, in, cost, t_max, eps, max_breaks);
        if (rc) return rc;
    }
    int status = LP_OPTIMAL;
    rc = bounded_parametric(ctx, in, dir, cost, nullptr, maximize, t_max, eps, max_breaks, out, &status, large);
    if (rc) return rc;
    if (status == LP_BAD_ARG) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the basis is not optimal at t = 0");
    return status;
}

// The batched entry of either path
static int bounded_parametric_many(lp_context* ctx, const char* who, bool cost, int batch, const double* A, int m,
                                   int n, const double* b, const double* c, const double* lo, const double* hi,
                                   const int* basis, const int* at_upper, const int* run_status, int maximize,
                                   const double* dir, double t_max, double eps, int max_breaks,
                                   const BoundedParametricOut& out, int* status_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !lo || !hi || !basis || !at_upper || !dir || !out.nseg || !out.t || !out.obj || !out.slope ||
        !out.enter || !out.leave || !out.side || !out.basis || !out.at_upper || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (batch <= 0 || m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    const BoundedSensIn in{batch, m, n, A, b, c, lo, hi, basis, at_upper};
    const int rc = bounded_parametric_args(ctx, who, in, cost, t_max, eps, max_breaks);
    if (rc) return rc;
    return bounded_parametric(ctx, in, dir, cost, run_status, maximize, t_max, eps, max_breaks, out, status_out);
}

int lp_basis_bounded_parametric(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                const double* lo, const double* hi, const int* basis, const int* at_upper,
                                int maximize, const double* d, double t_max, double eps, int max_breaks,
                                int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                                int* leave_out, int* side_out, int* basis_out, int* at_upper_out) {
    return bounded_parametric_one(ctx, "lp_basis_bounded_parametric", false, false, A, m, n, b, c, lo, hi, basis, at_upper,
                                  maximize, d, t_max, eps, max_breaks,
                                  {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, side_out, basis_out,
                                   at_upper_out});
}

int lp_basis_bounded_parametric_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                        const double* c, const double* lo, const double* hi, const int* basis,
                                        const int* at_upper, const int* run_status, int maximize, const double* d,
                                        double t_max, double eps, int max_breaks, int* nseg_out, double* t_out,
                                        double* obj_out, double* slope_out, int* enter_out, int* leave_out,
                                        int* side_out, int* basis_out, int* at_upper_out, int* status_out) {
    return bounded_parametric_many(ctx, "lp_basis_bounded_parametric_batched", false, batch, A, m, n, b, c, lo, hi,
                                   basis, at_upper, run_status, maximize, d, t_max, eps, max_breaks,
                                   {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, side_out, basis_out,
                                    at_upper_out}, status_out);
}

int lp_basis_bounded_parametric_cost(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                     const double* lo, const double* hi, const int* basis, const int* at_upper,
                                     int maximize, const double* g, double t_max, double eps, int max_breaks,
                                     int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                                     int* leave_out, int* side_out, int* basis_out, int* at_upper_out) {
    return bounded_parametric_one(ctx, "lp_basis_bounded_parametric_cost", false, true, A, m, n, b, c, lo, hi, basis,
                                  at_upper, maximize, g, t_max, eps, max_breaks,
                                  {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, side_out, basis_out,
                                   at_upper_out});
}

int lp_basis_bounded_parametric_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                      const double* lo, const double* hi, const int* basis, const int* at_upper,
                                      int maximize, const double* d, double t_max, double eps, int max_breaks,
                                      int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out,
                                      int* leave_out, int* side_out, int* basis_out, int* at_upper_out) {
    return bounded_parametric_one(ctx, "lp_basis_bounded_parametric_large", true, false, A, m, n, b, c, lo, hi, basis,
                                  at_upper, maximize, d, t_max, eps, max_breaks,
                                  {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, side_out, basis_out,
                                   at_upper_out});
}

int lp_basis_bounded_parametric_cost_large(lp_context* ctx, const double* A, int m, int n, const double* b,
                                           const double* c, const double* lo, const double* hi, const int* basis,
                                           const int* at_upper, int maximize, const double* g, double t_max,
                                           double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out,
                                           double* slope_out, int* enter_out, int* leave_out, int* side_out,
                                           int* basis_out, int* at_upper_out) {
    return bounded_parametric_one(ctx, "lp_basis_bounded_parametric_cost_large", true, true, A, m, n, b, c, lo, hi,
                                  basis, at_upper, maximize, g, t_max, eps, max_breaks,
                                  {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, side_out, basis_out,
                                   at_upper_out});
}

int lp_basis_bounded_parametric_cost_batched(lp_context* ctx, int batch, const double* A, int m, int n,
                                             const double* b, const double* c, const double* lo, const double* hi,
                                             const int* basis, const int* at_upper, const int* run_status,
                                             int maximize, const double* g, double t_max, double eps, int max_breaks,
                                             int* nseg_out, double* t_out, double* obj_out, double* slope_out,
                                             int* enter_out, int* leave_out, int* side_out, int* basis_out,
                                             int* at_upper_out, int* status_out) {
    return bounded_parametric_many(ctx, "lp_basis_bounded_parametric_cost_batched", true, batch, A, m, n, b, c, lo,
                                   hi, basis, at_upper, run_status, maximize, g, t_max, eps, max_breaks,
                                   {nseg_out, t_out, obj_out, slope_out, enter_out, leave_out, side_out, basis_out,
                                    at_upper_out}, status_out);
}

// ===========================================================================
// Depth-first branch-and-bound (batched_mip.hip): one integer LP per workgroup for lp_mip_fits shapes only; there is
// no per-LP path
// ===========================================================================

int lp_mip_fits(int m, int n, int max_depth) { return lp_mip_fits_shape(m, n, max_depth) ? 1 : 0; }


}  // extern "C"

// The search parameters and the mask, for both searches (max_depth in [0, depth_cap]).
int lp_mip_check_search(lp_context* ctx, const char* who, int n, int n_orig, const int* integer, double int_tol,
                        double gap, int max_depth, int depth_cap, int max_nodes) {
    if (!integer) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (max_depth < 0 || max_depth > depth_cap)
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": max_depth must be in [0, " + std::to_string(depth_cap) + "]");
    if (!(int_tol >= 0.0 && int_tol < 0.5)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": int_tol must be in [0, 0.5)");
    if (!(gap >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": gap must be >= 0");
    if (max_nodes < 1) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": max_nodes must be >= 1");
    for (int j = 0; j < n; ++j) {
        if (integer[j] != 0 && integer[j] != 1) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": mask entries must be 0 or 1");
        if (integer[j] && j >= n_orig)
            LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the mask marks a column beyond n_orig");
    }
    return LP_OPTIMAL;
}

extern "C" {

// The search parameters, the mask and the fit (the basis and the problem arrays are checked by the callers).
static int mip_args(lp_context* ctx, const char* who, int m, int n, int n_orig, const int* integer, double int_tol,
                    double gap, int max_depth, int max_nodes) {
    const int rc = lp_mip_check_search(ctx, who, n, n_orig, integer, int_tol, gap, max_depth, LP_MIP_MAX_DEPTH, max_nodes);
    if (rc) return rc;
    if (!lp_mip_fits_shape(m, n, max_depth))
        LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the shape does not fit one CU's LDS (lp_mip_fits)");
    return LP_OPTIMAL;
}

// The search of `batch` problems whose A, b, c and root bases are on the device: problems whose run status is not
// LP_OPTIMAL keep it.  The mask goes up.
static int mip_on_device(lp_context* ctx, int batch, int m, int n, int n_orig, const BasisInputs& in,
                         const int* integer, int maximize, double eps, double int_tol, double gap, int max_depth,
                         int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out,
                         int* found_out, int* stats_out, int* status_out) {
    const size_t B = (size_t)batch;
    lp_device_buffer buf;
    LP_HIP(ctx, hipMalloc(&buf.ptr, sizeof(double) * (B * n_orig + 2 * B) + sizeof(int) * (B * 6 + n)));
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
    d.A = in.A;
    d.b = in.b;
    d.c = in.c;
    d.basis_in = in.basis;
    d.run_status = in.run_status;
    d.x = reinterpret_cast<double*>(buf.ptr);
    d.obj = d.x + B * n_orig;
    d.bound = d.obj + B;
    d.found = reinterpret_cast<int*>(d.bound + B);
    d.stats = d.found + B;
    d.status = d.stats + B * 4;
    int* dmask = d.status + B;
    d.integer = dmask;
    hipError_t e = hipMemcpyAsync(dmask, integer, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched MIP upload: ") + hipGetErrorString(e));
    const int rc = lp_batched_mip_launch(ctx, d);
    if (rc) return rc;
    e = hipGetLastError();
    if (e != hipSuccess) LP_FAIL(ctx, -(int)e, std::string("batched MIP: ") + hipGetErrorString(e));
    return lp_download(ctx, "batched MIP", {{x_out, d.x, sizeof(double) * B * n_orig},
                                            {obj_out, d.obj, sizeof(double) * B},
                                            {bound_out, d.bound, sizeof(double) * B},
                                            {found_out, d.found, sizeof(int) * B},
                                            {stats_out, d.stats, sizeof(int) * B * 4},
                                            {status_out, d.status, sizeof(int) * B}});
}

int lp_mip_solve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const int* basis,
                 int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth,
                 int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out,
                 int* stats_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_solve: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_solve: eps must be >= 0");
    int rc = check_canonical(ctx, A, m, n, b, c, basis, n_orig);
    if (rc) return rc;
    rc = mip_args(ctx, "lp_mip_solve", m, n, n_orig, integer, int_tol, gap, max_depth, max_nodes);
    if (rc) return rc;
    lp_device_buffer buf;
    BasisInputs in;
    int status = LP_OPTIMAL;
    rc = upload(ctx, "batched MIP", buf, 1, m, n, A, b, c, nullptr, 0, basis, nullptr, in);
    if (rc == LP_OPTIMAL)
        rc = mip_on_device(ctx, 1, m, n, n_orig, in, integer, maximize, eps, int_tol, gap, max_depth, max_nodes,
                           max_iter, x_out, obj_out, bound_out, found_out, stats_out, &status);
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
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_solve_batched: eps must be >= 0");
    if (batch <= 0) LP_FAIL(ctx, LP_BAD_ARG, "batch must be positive");
    for (int k = 0; k < batch; ++k) {
        int rc = check_canonical(ctx, A ? A + (size_t)k * m * n : nullptr, m, n, b ? b + (size_t)k * m : nullptr,
                                 c ? c + (size_t)k * n : nullptr, basis ? basis + (size_t)k * m : nullptr, n_orig);
        if (rc) return rc;
    }
    int rc = mip_args(ctx, "lp_mip_solve_batched", m, n, n_orig, integer, int_tol, gap, max_depth, max_nodes);
    if (rc) return rc;
    lp_device_buffer buf;
    BasisInputs in;
    rc = upload(ctx, "batched MIP", buf, batch, m, n, A, b, c, nullptr, 0, basis, nullptr, in);
    return rc ? rc
              : mip_on_device(ctx, batch, m, n, n_orig, in, integer, maximize, eps, int_tol, gap, max_depth,
                              max_nodes, max_iter, x_out, obj_out, bound_out, found_out, stats_out, status_out);
}

int lp_batched_mip(lp_batched_problem* p, const int* integer, double eps, double int_tol, double gap, int max_depth,
                   int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out,
                   int* stats_out, int* status_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out || !status_out)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_mip: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_mip: eps must be >= 0");
    int rc = mip_args(ctx, "lp_batched_mip", p->m, p->n, p->n_orig, integer, int_tol, gap, max_depth, max_nodes);
    if (rc) return rc;
    if (p->pivot_rule != LP_PIVOT_DANTZIG) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_mip: Dantzig's rule only");
    if (!p->ran) LP_FAIL(ctx, LP_BAD_ARG, "lp_batched_mip: the batch has not run");
    lp_device_buffer buf;
    BasisInputs in;
    rc = batch_inputs(p, "batched MIP", buf, nullptr, 0, in);
    return rc ? rc
              : mip_on_device(ctx, p->batch, p->m, p->n, p->n_orig, in, integer, p->maximize, eps, int_tol, gap,
                              max_depth, max_nodes, max_iter, x_out, obj_out, bound_out, found_out, stats_out,
                              status_out);
}

}  // extern "C"
