// simplex_driver.hip — the host side of the single-LP simplex: upload and download, the dispatch among the four
// algorithms, the batch-and-poll loop three of them share, the epilogue that fills lp_simplex_stats, the two-phase
// flow and the update micro-benchmarks.  The algorithm files (simplex_launch / _lookahead / _overlap / _resident.hip)
// hold the kernels and the small launch surface declared in simplex_problem.hpp.  The bounded-variable entries on the
// same tableau (simplex_bounded_driver.hip) use the upload, the polling loop and the two-phase pieces of this file.
#include <chrono>
#include <cmath>
#include <cstdio>

#include "lp_internal.hpp"
#include "simplex_problem.hpp"

// Canonical's constructor checks (Canonical.cpp:27-46) + SetOriginalVariablesCount (:156-163).
int check_canonical(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                    const int* basis, int n_orig) {
    if (!A || !b || !c || !basis) LP_FAIL(ctx, LP_BAD_ARG, "null problem array");
    if (m <= 0 || n <= 0) LP_FAIL(ctx, LP_BAD_ARG, "empty problem");
    if (n < m) LP_FAIL(ctx, LP_BAD_ARG, "fewer columns than rows");
    if (n_orig <= 0 || n_orig > n) LP_FAIL(ctx, LP_BAD_ARG, "bad original variable count");
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) LP_FAIL(ctx, LP_BAD_ARG, "basis index out of range");
    return LP_OPTIMAL;
}

void lp_slack_identity(const double* A, int m, const double* c, const int* basis, bool* identity, bool* zero_costs,
                       const int* at_upper) {
    bool id = true, zero = true;
    for (int t = 0; t < m && id; ++t) {
        if (c[basis[t]] != 0.0) zero = false;
        const bool negated = at_upper && at_upper[basis[t]];
        const double* col = A + (size_t)basis[t] * m;
        for (int i = 0; i < m && id; ++i)
            if ((negated ? -col[i] : col[i]) != ((i == t) ? 1.0 : 0.0)) id = false;
    }
    *identity = id;
    *zero_costs = zero;
}

hipError_t lp_lds_opt_in(const void* kernel, size_t bytes) {
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

namespace {

constexpr int kRunning = -100;  // SimplexState::status while pivoting

// ---- one run: the batch-and-poll loop and the epilogue shared by the paths

// Queues pivots in batches of first, 2 first, ... up to cap and polls the state word once per batch until it
// leaves kRunning (the kernels turn into no-ops once it has).  queue(batch) returns the launches it queued.
template <class Queue>
int poll_batches(lp_simplex_problem* p, int first, int cap, int* launches, Queue queue) {
    lp_context* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    for (int batch = first;; batch = std::min(2 * batch, cap)) {
        const int queued = queue(batch);
        if (queued < 0) return queued;
        *launches += queued;
        LP_HIP(ctx, hipGetLastError());   // a refused launch leaves the state word at kRunning: never poll on it
        LP_HIP(ctx, hipMemcpyAsync(p->h_state, p->dev.state, sizeof(SimplexState), hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipStreamSynchronize(s));
        if (p->h_state->status != kRunning) return LP_OPTIMAL;
    }
}

// Closes the timed window: ev1 behind everything queued; *ms = the whole solve.
int close_window(lp_simplex_problem* p, float* ms) {
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipEventRecord(p->ev1, ctx->stream));
    LP_HIP(ctx, hipEventSynchronize(p->ev1));
    LP_HIP(ctx, hipGetLastError());
    LP_HIP(ctx, hipEventElapsedTime(ms, p->ev0, p->ev1));
    return LP_OPTIMAL;
}

// The outcome of a run from the state word: last_* and the stats record.  Returns the status.
int record_run(lp_simplex_problem* p, int algo, int launches, float ms, float update_ms, int update_launches,
               lp_simplex_stats* stats) {
    const SimplexDev& d = p->dev;
    const int status = p->h_state->status;
    p->last_status = status;
    p->last_iters = p->h_state->iters;
    p->last_algo = algo;
    if (stats) {
        stats->status = status;
        stats->pivots = p->h_state->iters;
        stats->launches = launches;
        stats->solve_ms = ms;
        stats->update_ms = update_ms;
        stats->update_launches = update_launches;
        stats->bytes_per_pivot = 16.0 * (double)d.m * (double)(d.n + 1);
    }
    return status;
}

// A select + rank-1 update launch pair per pivot, polled in batches: prepare(p) opts the selector's LDS in, queue(p,
// batch) queues the pairs.  The selector of p->pivot_rule, or the pair passed (lp_simplex_resolve_run: the dual one).
int run_launch(lp_simplex_problem* p, double eps, int max_iter, lp_simplex_stats* stats,
               int (*prepare)(lp_simplex_problem*) = lp_launch_prepare,
               int (*queue)(lp_simplex_problem*, int) = lp_launch_queue) {
    int rc = prepare(p);
    if (rc) return rc;
    LP_HIP(p->ctx, hipEventRecord(p->ev0, p->ctx->stream));
    int launches = lp_launch_begin(p, eps, max_iter);
    rc = poll_batches(p, 16, 256, &launches, [&](int batch) { return queue(p, batch); });
    if (rc) return rc;
    float ms = 0.f;
    rc = close_window(p, &ms);
    if (rc) return rc;
    return record_run(p, LP_SIMPLEX_ALGO_LAUNCH, launches, ms, 0.f, 0, stats);
}

int run_lookahead(lp_simplex_problem* p, double eps, int max_iter, lp_simplex_stats* stats) {
    lp_context* ctx = p->ctx;
    int rc = lp_lookahead_prepare(p);
    if (rc) return rc;
    LP_HIP(ctx, hipEventRecord(p->ev0, ctx->stream));
    int launches = lp_lookahead_begin(p, eps, max_iter);
    // HIP events around the first kMaxTimed rank-J update launches (the kernel the HBM roofline
    // is quoted on); launches after termination are no-ops and are not counted.
    constexpr int kMaxTimed = 512;
    if (p->upd_events.empty()) {
        p->upd_events.resize(2 * kMaxTimed);
        for (auto& e : p->upd_events) LP_HIP(ctx, hipEventCreate(&e));
    }
    int timed = 0;
    rc = poll_batches(p, 4, 64, &launches, [&](int batch) { return lp_lookahead_queue(p, batch, &timed); });
    if (rc) return rc;
    float ms = 0.f, upd = 0.f;
    rc = close_window(p, &ms);
    if (rc) return rc;
    // update launches that did real work: one per started batch of J pivots
    const int real = std::min((p->h_state->iters + p->look.J - 1) / p->look.J, timed);
    if (stats)
        for (int k = 0; k < real; ++k) {
            float t = 0.f;
            LP_HIP(ctx, hipEventElapsedTime(&t, p->upd_events[2 * k], p->upd_events[2 * k + 1]));
            upd += t;
        }
    return record_run(p, LP_SIMPLEX_ALGO_LOOKAHEAD, launches, ms, upd, real, stats);
}

int run_overlap(lp_simplex_problem* p, double eps, int max_iter, lp_simplex_stats* stats) {
    int rc = lp_overlap_prepare(p);
    if (rc) return rc;
    OverlapPlan plan;
    rc = lp_overlap_plan(p, &plan);
    if (rc) return rc;
    LP_HIP(p->ctx, hipEventRecord(p->ev0, p->ctx->stream));
    int launches = lp_overlap_begin(p, eps, max_iter);
    rc = poll_batches(p, 16, 256, &launches, [&](int batch) { return lp_overlap_queue(p, plan, batch); });
    if (rc) return rc;
    rc = lp_overlap_finish(p);
    if (rc) return rc;
    float ms = 0.f;
    rc = close_window(p, &ms);
    if (rc) return rc;
    return record_run(p, LP_SIMPLEX_ALGO_OVERLAP, launches, ms, 0.f, 0, stats);
}

int run_resident(lp_simplex_problem* p, double eps, int max_iter, lp_simplex_stats* stats) {
    lp_context* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    LP_HIP(ctx, hipEventRecord(p->ev0, s));
    int rc = lp_resident_launch(p, eps, max_iter);
    if (rc) return rc;
    LP_HIP(ctx, hipMemcpyAsync(p->h_state, p->dev.state, sizeof(SimplexState), hipMemcpyDeviceToHost, s));
    float ms = 0.f, kms = 0.f;
    rc = close_window(p, &ms);
    if (rc) return rc;
    LP_HIP(ctx, hipEventElapsedTime(&kms, p->res_ev0, p->res_ev1));
    bool rerun = false;
    rc = lp_resident_finish(p, &rerun);
    if (rc) return rc;
    if (!rerun) return record_run(p, LP_SIMPLEX_ALGO_RESIDENT, 2, ms, kms, 1, stats);
    // The time-out fallback and AUTO's rule (lp_simplex_run) differ on purpose.  The fallback chooses between the
    // look-ahead path and the launch pair only, so it takes the look-ahead path from depth 2 on; AUTO also has the
    // overlapped path, which beats depth 2 (1536 x 3072: 18.4 us per pivot against 20.0), so it needs depth 3.
    rc = p->look.J >= 2 ? run_lookahead(p, eps, max_iter, stats) : run_launch(p, eps, max_iter, stats);
    if (rc >= 0 && stats) stats->solve_ms += ms;   // the caller waited for the timed-out launch too
    return rc;
}

// ---- update micro-benchmarks

// Saves the tableau to dscratchT, stages a pivot (stage), replays `launch` three times to warm up and then `iters`
// times between ev0 and ev1, and puts the tableau back; restore queues whatever else the staging changed.  The
// replays re-apply the same eta, so the values drift: irrelevant for timing.
template <class Stage, class Launch, class Restore>
int bench_replay(lp_simplex_problem* p, int iters, float* ms_per_launch, Stage stage, Launch launch, Restore restore) {
    lp_context* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    if (!p->dscratchT) LP_HIP(ctx, hipMalloc(&p->dscratchT, p->tableau_bytes));   // (micro-benchmarks only)
    LP_HIP(ctx, hipMemcpyAsync(p->dscratchT, p->dev.T, p->tableau_bytes, hipMemcpyDeviceToDevice, s));
    int rc = stage();
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) launch();
    LP_HIP(ctx, hipEventRecord(p->ev0, s));
    for (int k = 0; k < iters; ++k) launch();
    LP_HIP(ctx, hipEventRecord(p->ev1, s));
    LP_HIP(ctx, hipEventSynchronize(p->ev1));
    float ms = 0.f;
    LP_HIP(ctx, hipEventElapsedTime(&ms, p->ev0, p->ev1));
    if (ms_per_launch) *ms_per_launch = ms / (float)iters;
    LP_HIP(ctx, hipMemcpyAsync(p->dev.T, p->dscratchT, p->tableau_bytes, hipMemcpyDeviceToDevice, s));
    rc = restore();
    if (rc) return rc;
    LP_HIP(ctx, hipStreamSynchronize(s));
    LP_HIP(ctx, hipGetLastError());
    return LP_OPTIMAL;
}

}  // namespace

int lp_poll_pivots(lp_simplex_problem* p, const std::function<int(int)>& queue) {
    int launches = 0;
    return poll_batches(p, 16, 256, &launches, queue);
}

// ---- the two-phase flow shared by lp_simplex_two_phase_ex and lp_simplex_bounded_large (simplex_bounded_driver.hip)

// make_b_nonneg (:61-68) and createAuxiliaryProblem (:70-95) on [A | b]: rows with b_i < -eps change sign, an identity
// of artificials with cost 1 follows A, and they are the starting basis.  A1 (m x (n+m), column-major) and c1 (n+m)
// come zeroed; b1 may be b itself (lp_simplex_bounded_large's shifted right-hand side).
void auxiliary_problem(const double* A, int m, int n, const double* b, double eps, double* A1, double* b1, double* c1,
                       int* N) {
    std::vector<char> flip((size_t)m);
    for (int i = 0; i < m; ++i) {
        flip[(size_t)i] = b[i] < -eps;
        b1[i] = flip[(size_t)i] ? -b[i] : b[i];
        A1[(size_t)(n + i) * m + i] = 1.0;
        c1[n + i] = 1.0;
        N[i] = n + i;
    }
    for (int j = 0; j < n; ++j) {   // (column by column: both matrices are column-major)
        const double* src = A + (size_t)j * m;
        double* dst = A1 + (size_t)j * m;
        for (int i = 0; i < m; ++i) dst[i] = flip[(size_t)i] ? -src[i] : src[i];
    }
}

// Phase I's verdict (:347-353): the artificials' values, summed in artificial-index order, against eps
int phase1_verdict(lp_context* ctx, const std::string& prefix, const double* xa, int m, int n, double eps) {
    double sum = 0.0;
    for (int i = 0; i < m; ++i) sum += xa[(size_t)n + i];
    if (!(sum > eps)) return LP_OPTIMAL;
    ctx->last_error = prefix + ": the problem has no feasible solution (phase I optimum > eps)";
    return LP_INFEASIBLE;
}

// The positions of the phase-I basis N that still hold an artificial
static std::vector<int> artificial_positions(const int* N, int m, int n) {
    std::vector<int> positions;
    for (int pos = 0; pos < m; ++pos)
        if (N[pos] >= n) positions.push_back(pos);
    return positions;
}

// replaceArtificialColumns (:331-381): every artificial still basic (at level 0) leaves for the first non-basic
// original column with |T[pos][cand]| > eps, chosen on the device; the positions are known from the phase-I basis, so
// all pivots are queued behind one another.  No bound enters it.
int drive_out_artificials(lp_simplex_problem* p, const std::string& prefix, const int* N, int m, int n, double eps,
                          int* pivots) {
    const std::vector<int> positions = artificial_positions(N, m, n);
    if (positions.empty()) return LP_OPTIMAL;
    const int rc = lp_simplex_driveout(p, positions.data(), (int)positions.size(), n, eps, pivots);
    if (rc == LP_SINGULAR)   // :372-380: linearly dependent constraints
        p->ctx->last_error = prefix + ": an artificial variable cannot leave the basis (linearly dependent constraints)";
    return rc;
}

// After a positive status: the basis reached, as the one-LP-per-workgroup kernels report it
int download_basis(lp_simplex_problem* p, int* N) {
    return lp_simplex_download(p, nullptr, N, nullptr, nullptr, nullptr, 0, nullptr);
}

extern "C" {

void lp_simplex_free(lp_simplex_problem* p) {
    if (!p) return;
    lp_context* ctx = p->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);   // the arena goes back to the pool: nothing may still use it
    lp_pool_release(ctx, p->arena, p->arena_bytes);
    (void)hipFree(p->dscratchT);
    (void)hipFree(p->ov_T);
    (void)hipFree(p->ov_vec);
    (void)hipFree(p->dweights);
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

}  // extern "C"

// The problem record of an m x n tableau with every device buffer behind it (one arena from the context's pool), the
// pinned state block and the events; nothing is uploaded.  c (n, may be null): the costs lp_simplex_download evaluates.
int lp_simplex_alloc(lp_context* ctx, int m, int n, const double* c, int maximize, int n_orig,
                     lp_simplex_problem** problem_out) {
    *problem_out = nullptr;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    // every error return below frees the half-built problem
    std::unique_ptr<lp_simplex_problem, void (*)(lp_simplex_problem*)> owner(new lp_simplex_problem(), lp_simplex_free);
    lp_simplex_problem* p = owner.get();
    p->ctx = ctx;
    p->n_orig = n_orig;
    if (c) p->h_c.assign(c, c + n);
    SimplexDev& d = p->dev;
    d.m = m;
    d.n = n;
    d.ld = ((n + 1 + 7) / 8) * 8;
    d.maximize = maximize ? 1 : 0;
    d.trace_cap = 16384;
    const size_t rows = (size_t)m + 1;
    p->tableau_bytes = sizeof(double) * rows * (size_t)d.ld;
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
        LP_HIP(ctx, lp_pool_alloc(ctx, &p->arena, off, &got));
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
        LP_HIP(ctx, hipHostMalloc(&p->h_state, sizeof(SimplexState) + 64));
        LP_HIP(ctx, hipEventCreate(&p->ev0));
        LP_HIP(ctx, hipEventCreate(&p->ev1));
    }
    LP_HIP(ctx, hipMemsetAsync(la.count, 0, sizeof(int), ctx->stream));
    *problem_out = owner.release();
    return LP_OPTIMAL;
}

// The tail of an upload: the tableau [A | b] with the cost row c underneath from the column-major A, b and c staged
// in p->dT0 (A first, then b, then c), the basis, and computeBFS; the post-crash snapshot goes back into p->dT0.
// identity / zero_costs: lp_slack_identity's verdict on the staged problem.  Sets p->init_status.
int lp_simplex_install(lp_simplex_problem* p, const int* basis_in, bool identity, bool zero_costs) {
    lp_context* ctx = p->ctx;
    const SimplexDev& d = p->dev;
    const int m = d.m, n = d.n;
    hipStream_t s = ctx->stream;
    const double* dA = p->dT0;
    const double* db = dA + (size_t)m * n;
    const double* dc = db + m;
    std::vector<unsigned char> nonbasic((size_t)n, 1);
    for (int t = 0; t < m; ++t) nonbasic[(size_t)basis_in[t]] = 0;
    hipLaunchKernelGGL(k_build_tableau, dim3(lp_ceil_div(n, 32), lp_ceil_div(m, 32)), 256, 0, s, dA, db, dc, d.T, m, n,
                       d.ld);
    LP_HIP(ctx, hipMemcpyAsync(d.basis, basis_in, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(p->dbasis0, basis_in, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(d.nonbasic, nonbasic.data(), (size_t)n, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(p->dnonbasic0, nonbasic.data(), (size_t)n, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipStreamSynchronize(s));
    LP_HIP(ctx, hipGetLastError());

    // computeBFS (SimplexSolover.h:423): nothing to do for the slack identity basis with
    // zero basic costs (Symmetrical::ToCanonical, Symmetrical.cpp:169-188); otherwise m
    // Gauss-Jordan pivots on the device.
    p->init_status = LP_OPTIMAL;
    if (identity && !zero_costs) {
        // unit-vector basis with costs (the artificial basis of a phase-I problem): the crash pivots
        // only touch the reduced-cost row — one pass instead of m rank-1 updates
        const int rc = lp_simplex_price_out_identity(p);
        if (rc) return rc;
    } else if (!identity) {
        const int rc = lp_simplex_crash(p);
        if (rc < 0) return rc;
        p->init_status = rc;
    }
    LP_HIP(ctx, hipMemcpyAsync(p->dT0, d.T, p->tableau_bytes, hipMemcpyDeviceToDevice, s));
    LP_HIP(ctx, hipStreamSynchronize(s));
    return LP_OPTIMAL;
}

extern "C" {

int lp_simplex_upload(lp_context* ctx, const double* A, int m, int n, const double* b,
                      const double* c, const int* basis_in, int maximize, int n_orig,
                      lp_simplex_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    int rc = check_canonical(ctx, A, m, n, b, c, basis_in, n_orig);
    if (rc) return rc;
    lp_simplex_problem* p = nullptr;
    rc = lp_simplex_alloc(ctx, m, n, c, maximize, n_orig, &p);
    if (rc) return rc;
    ProblemOwner owner(p, lp_simplex_free);   // every error return below frees the half-built problem
    // A goes up as the caller holds it (column-major) into the staging area and is transposed on the device
    hipStream_t s = ctx->stream;
    double* dA = p->dT0;
    double* db = dA + (size_t)m * n;
    double* dc = db + m;
    LP_HIP(ctx, hipMemcpyAsync(dA, A, sizeof(double) * (size_t)m * n, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(db, b, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(dc, c, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    bool identity, zero_costs;
    lp_slack_identity(A, m, c, basis_in, &identity, &zero_costs);
    rc = lp_simplex_install(p, basis_in, identity, zero_costs);
    if (rc) return rc;
    *problem_out = owner.release();
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
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_run: eps must be >= 0");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
    if (p->init_status != LP_OPTIMAL) {  // "Singular basis matrix", SimplexSolover.h:125-126
        if (stats_out) stats_out->status = p->init_status;
        p->last_status = p->init_status;
        return p->init_status;
    }
    const bool asked_auto = algo == LP_SIMPLEX_ALGO_AUTO;
    const bool bland = p->pivot_rule == LP_PIVOT_BLAND;
    if (bland || p->pivot_rule == LP_PIVOT_DEVEX) {   // Bland's and the Devex selector exist for the launch pair only
        if (algo == LP_SIMPLEX_ALGO_AUTO) algo = LP_SIMPLEX_ALGO_LAUNCH;
        if (algo == LP_SIMPLEX_ALGO_RESIDENT || algo == LP_SIMPLEX_ALGO_LOOKAHEAD || algo == LP_SIMPLEX_ALGO_OVERLAP)
            LP_FAIL(ctx, LP_BAD_ARG, bland ? "Bland's pivot rule runs on LP_SIMPLEX_ALGO_LAUNCH (or AUTO) only"
                                           : "Devex pricing runs on LP_SIMPLEX_ALGO_LAUNCH (or AUTO) only");
    }
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
            rc = run_resident(p, eps, max_iter, stats_out);
            break;
        case LP_SIMPLEX_ALGO_LAUNCH:
            rc = run_launch(p, eps, max_iter, stats_out);
            break;
        case LP_SIMPLEX_ALGO_OVERLAP:
            rc = run_overlap(p, eps, max_iter, stats_out);
            break;
        case LP_SIMPLEX_ALGO_LOOKAHEAD:
            if (p->look.J < 1)
                LP_FAIL(ctx, LP_BAD_ARG, "look-ahead selector does not fit LDS for this m, n");
            rc = run_lookahead(p, eps, max_iter, stats_out);
            break;
        default:
            LP_FAIL(ctx, LP_BAD_ARG, "unknown simplex algorithm id");
    }
    if (stats_out) {   // which algorithm produced the answer (a chip-resident hand-off that timed out is re-run)
        stats_out->algo_used = p->last_algo;
        stats_out->fell_back = (asked == LP_SIMPLEX_ALGO_RESIDENT && p->last_algo != LP_SIMPLEX_ALGO_RESIDENT) ? 1 : 0;
    }
    return rc;
}

int lp_simplex_resolve_run(lp_simplex_problem* p, double eps, int max_iter, int* iters_out,
                           lp_simplex_stats* stats_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_resolve_run: eps must be >= 0");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
    if (iters_out) iters_out[0] = iters_out[1] = 0;
    if (p->pivot_rule != LP_PIVOT_DANTZIG) LP_FAIL(ctx, LP_BAD_ARG, "the re-solve runs Dantzig's rule only");
    if (p->init_status != LP_OPTIMAL) {   // the crash found the basis singular
        if (stats_out) stats_out->status = p->init_status;
        p->last_status = p->init_status;
        return p->init_status;
    }
    int flags = 0;
    int rc = lp_simplex_classify(p, eps, &flags);
    if (rc) return rc;
    if (!(flags & 1)) {   // primal feasible: the plain solve, every algorithm AUTO may pick
        rc = lp_simplex_run(p, eps, max_iter, LP_SIMPLEX_ALGO_AUTO, stats_out);
        if (iters_out && rc >= 0) iters_out[1] = p->last_iters;
        return rc;
    }
    if (flags & 2) LP_FAIL(ctx, LP_BAD_ARG, "re-solve: the basis is neither primal nor dual feasible");
    rc = run_launch(p, eps, max_iter, stats_out, lp_dual_prepare, lp_dual_queue);   // the dual selector's pair
    if (stats_out) {
        stats_out->algo_used = LP_SIMPLEX_ALGO_LAUNCH;
        stats_out->fell_back = 0;
    }
    if (iters_out && rc >= 0) iters_out[0] = p->last_iters;
    return rc;
}

int lp_simplex_set_pivot_rule(lp_simplex_problem* p, int pivot_rule) {
    if (!p) return LP_BAD_ARG;
    if (!lp_pivot_rule_known(pivot_rule))
        LP_FAIL(p->ctx, LP_BAD_ARG, "unknown pivot rule");
    p->pivot_rule = pivot_rule;
    return LP_OPTIMAL;
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
    return lp_simplex_solve_ex(ctx, A, m, n, b, c, basis_in, maximize, n_orig, eps, max_iter, x_out, basis_out,
                               obj_out, iters_out, LP_PIVOT_DANTZIG);
}

int lp_simplex_solve_ex(lp_context* ctx, const double* A, int m, int n, const double* b,
                        const double* c, const int* basis_in, int maximize, int n_orig, double eps,
                        int max_iter, double* x_out, int* basis_out, double* obj_out, int* iters_out,
                        int pivot_rule) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out) LP_FAIL(ctx, LP_BAD_ARG, "x_out is null");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_solve: eps must be >= 0");
    if (!lp_pivot_rule_known(pivot_rule)) LP_FAIL(ctx, LP_BAD_ARG, "unknown pivot rule");
    lp_simplex_problem* p = nullptr;
    int rc = lp_simplex_upload(ctx, A, m, n, b, c, basis_in, maximize, n_orig, &p);
    if (rc) return rc;
    p->pivot_rule = pivot_rule;
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

int lp_simplex_resolve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                       const int* basis_in, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                       int* basis_out, double* obj_out, int* iters_out) {
    if (!ctx) return LP_BAD_ARG;
    if (!x_out) LP_FAIL(ctx, LP_BAD_ARG, "x_out is null");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_resolve: eps must be >= 0");
    if (iters_out) iters_out[0] = iters_out[1] = 0;
    lp_simplex_problem* p = nullptr;
    int rc = lp_simplex_upload(ctx, A, m, n, b, c, basis_in, maximize, n_orig, &p);
    if (rc) return rc;
    rc = lp_simplex_resolve_run(p, eps, max_iter, iters_out, nullptr);
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
    return lp_simplex_two_phase_ex(ctx, A, m, n, b, c, maximize, n_orig, eps, max_iter, x_out, basis_out, obj_out,
                                   iters_out, LP_PIVOT_DANTZIG);
}

int lp_simplex_two_phase_ex(lp_context* ctx, const double* A, int m, int n, const double* b,
                            const double* c, int maximize, int n_orig, double eps, int max_iter,
                            double* x_out, int* basis_out, double* obj_out, int* iters_out,
                            int pivot_rule) {
    if (!ctx) return LP_BAD_ARG;
    if (!A || !b || !c || !x_out) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_two_phase: null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, "lp_simplex_two_phase: eps must be >= 0");
    if (!lp_pivot_rule_known(pivot_rule)) LP_FAIL(ctx, LP_BAD_ARG, "unknown pivot rule");
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
    auxiliary_problem(A, m, n, b, eps, A1.data(), b1.data(), c1.data(), N.data());
    stage("auxiliary problem (host)");
    // ---- phase I: minimise the sum of the artificials
    lp_simplex_problem* p = nullptr;
    int rc = lp_simplex_upload(ctx, A1.data(), m, na, b1.data(), c1.data(), N.data(), 0, na, &p);
    if (rc) return rc;
    ProblemOwner owner(p, lp_simplex_free);
    p->pivot_rule = pivot_rule;   // phase I and phase II; the drive-out has its own rule
    stage("upload");
    lp_simplex_stats st;
    rc = lp_simplex_run(p, eps, max_iter, LP_SIMPLEX_ALGO_AUTO, &st);
    it[0] = st.pivots;
    stage("phase I run");
    if (rc == LP_OPTIMAL) rc = lp_simplex_download(p, xa.data(), N.data(), nullptr, nullptr, nullptr, 0, nullptr);
    stage("phase I download");
    if (rc == LP_OPTIMAL) rc = phase1_verdict(ctx, "two-phase", xa.data(), m, n, eps);
    if (rc == LP_OPTIMAL) rc = drive_out_artificials(p, "two-phase", N.data(), m, n, eps, &it[1]);
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
            (void)download_basis(p, N.data());
    } else if (rc > 0) {   // (phase I's iteration limit too)
        (void)download_basis(p, N.data());
    }
    stage("phase II download");
    owner.reset();
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

// The rank-1 update alone, on a valid pivot staged with the crash selector's arithmetic; the tableau and the state
// word are restored afterwards.
int lp_bench_rank1_update(lp_simplex_problem* p, int row, int col, int iters,
                          float* ms_per_launch_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const SimplexDev& d = p->dev;
    hipStream_t s = ctx->stream;
    if (row < 0 || row >= d.m || col < 0 || col >= d.n || iters <= 0)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_bench_rank1_update: bad pivot position or iteration count");
    SimplexState hs;
    std::vector<double> lcol((size_t)d.m + 1), prow((size_t)d.ld);
    auto stage = [&]() -> int {
        std::vector<double> Th((size_t)(d.m + 1) * d.ld);
        LP_HIP(ctx, hipMemcpyAsync(Th.data(), d.T, p->tableau_bytes, hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipStreamSynchronize(s));
        const double ur = Th[(size_t)row * d.ld + col];
        if (ur == 0.0) LP_FAIL(ctx, LP_BAD_ARG, "lp_bench_rank1_update: zero pivot element");
        for (int i = 0; i <= d.m; ++i)
            lcol[i] = (i == row) ? 1.0 : -1e-3 * Th[(size_t)i * d.ld + col] / ur;  // damped: stays finite
        for (int j = 0; j < d.ld; ++j) prow[j] = Th[(size_t)row * d.ld + j];
        std::memset(&hs, 0, sizeof(hs));
        hs.status = kRunning;
        hs.enter = col;
        hs.leave = row;
        hs.pivot_valid = 1;
        LP_HIP(ctx, hipMemcpyAsync(d.lcol, lcol.data(), sizeof(double) * lcol.size(), hipMemcpyHostToDevice, s));
        LP_HIP(ctx, hipMemcpyAsync(d.prow, prow.data(), sizeof(double) * prow.size(), hipMemcpyHostToDevice, s));
        LP_HIP(ctx, hipMemcpyAsync(d.state, &hs, sizeof(hs), hipMemcpyHostToDevice, s));
        return LP_OPTIMAL;
    };
    auto restore = [&]() -> int {
        hs.status = p->last_status;
        hs.iters = p->last_iters;
        hs.pivot_valid = 0;
        LP_HIP(ctx, hipMemcpyAsync(d.state, &hs, sizeof(hs), hipMemcpyHostToDevice, s));
        return LP_OPTIMAL;
    };
    return bench_replay(p, iters, ms_per_launch_out, stage, [&] { lp_simplex_launch_update(p); }, restore);
}

// The rank-J update alone: one batch of J pivots staged by the selector on the current tableau; the tableau, the
// basis bookkeeping (the selector moved it) and the staged count are restored afterwards.
int lp_bench_rankj_update(lp_simplex_problem* p, int iters, float* ms_per_launch_out,
                          int* pivots_per_launch_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const SimplexDev& d = p->dev;
    hipStream_t s = ctx->stream;
    if (p->look.J < 1 || iters <= 0) LP_FAIL(ctx, LP_BAD_ARG, "look-ahead path unavailable for this problem");
    int rc = lp_lookahead_prepare(p);
    if (rc) return rc;
    int count = 0;
    auto stage = [&]() -> int {
        lp_lookahead_begin(p, 1e-9, 1 << 30);
        lp_lookahead_launch_select(p);
        LP_HIP(ctx, hipMemcpyAsync(&count, p->look.count, sizeof(int), hipMemcpyDeviceToHost, s));
        LP_HIP(ctx, hipStreamSynchronize(s));
        if (count <= 0) LP_FAIL(ctx, LP_BAD_ARG, "no pivot could be staged on the current tableau");
        return LP_OPTIMAL;
    };
    auto restore = [&]() -> int {
        LP_HIP(ctx, hipMemcpyAsync(d.basis, p->dbasis0, sizeof(int) * (size_t)d.m, hipMemcpyDeviceToDevice, s));
        LP_HIP(ctx, hipMemcpyAsync(d.nonbasic, p->dnonbasic0, (size_t)d.n, hipMemcpyDeviceToDevice, s));
        LP_HIP(ctx, hipMemsetAsync(p->look.count, 0, sizeof(int), s));
        return LP_OPTIMAL;
    };
    rc = bench_replay(p, iters, ms_per_launch_out, stage, [&] { lp_lookahead_launch_update(p); }, restore);
    if (rc == LP_OPTIMAL && pivots_per_launch_out) *pivots_per_launch_out = count;
    return rc;
}

}  // extern "C"
