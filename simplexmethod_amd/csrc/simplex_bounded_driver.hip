// simplex_bounded_driver.hip — the host side of the bounded-variable simplex on the tableau in HBM, for LPs beyond one
// workgroup's LDS: lp_simplex_bounded_large, lp_simplex_bounded_resolve_large (both also as _ex under a pivot rule, the
// re-solve as _dual_ex under a dual pricing rule and as _ratio_ex under a dual ratio test too) and lp_mip_bounded_solve_large (as _ex with tableau snapshots for
// the second children).  The selectors are simplex_bounded_launch.hip's, the search's kernels
// mip_bounded_large.hip's; the problem record, the upload and the two-phase pieces are simplex_driver.hip's.
#include <algorithm>
#include <cmath>

#include "batched_problem.hpp"   // lp_mip_check_search, LP_MIP_BOUNDED_MAX_DEPTH
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

// ---- the checks of an entry, in the order the references test (it decides which message a doubly bad input gets)

// What all three entries refuse before an output is touched: the context, the pivot rule (an entry without one passes
// LP_PIVOT_DANTZIG), a null among its pointers (any_null), eps, the dimensions, the bounds (lo finite, hi not NaN).
int check_bounded_entry(lp_context* ctx, const char* who, int pivot_rule, bool any_null, double eps, int m, int n,
                        int n_orig, const double* lo, const double* hi) {
    if (!ctx) return LP_BAD_ARG;
    if (!lp_pivot_rule_known(pivot_rule)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": unknown pivot rule");
    if (any_null) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": null argument");
    if (!(eps >= 0.0)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": eps must be >= 0");
    if (m <= 0 || n < m || n_orig <= 0 || n_orig > n) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": bad dimensions");
    for (int j = 0; j < n; ++j) {
        if (!std::isfinite(lo[j])) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": lo must be finite");
        if (std::isnan(hi[j])) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": hi is NaN");
    }
    return LP_OPTIMAL;
}

// What the two warm entries add: every flag 0 or 1 and set only under a finite hi, then every basis index in [0, n).
// (batched_driver.hip and basis_driver.hip keep their own: per LP of a batch, std::isinf(hi), and the fit tests.)
int check_bounded_start(lp_context* ctx, const char* who, int n, int m, const double* hi, const int* basis_in,
                        const int* at_upper_in) {
    for (int j = 0; j < n; ++j) {
        if (at_upper_in[j] != 0 && at_upper_in[j] != 1) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": at_upper must be 0 or 1");
        if (at_upper_in[j] && hi[j] == INFINITY) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": a column without an upper bound is flagged at_upper");
    }
    for (int t = 0; t < m; ++t)
        if (basis_in[t] < 0 || basis_in[t] >= n) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": basis index out of range");
    return LP_OPTIMAL;
}

// Any hi_j < lo_j: LP_INFEASIBLE with nothing launched
int check_crossed(lp_context* ctx, const char* who, const double* lo, const double* hi, int n) {
    for (int j = 0; j < n; ++j)
        if (hi[j] < lo[j]) LP_FAIL(ctx, LP_INFEASIBLE, std::string(who) + ": some hi_j < lo_j");
    return LP_OPTIMAL;
}

// ---- the pieces the solve and the re-solve share

// The shift chain: b1_i <- fma(-A_ij, w_j, b1_i) over the columns with take(j), per row in ascending j (column by
// column: A is column-major)
template <class Take>
void shift_rhs(const double* A, int m, int n, const double* w, Take take, double* b1) {
    for (int j = 0; j < n; ++j) {
        if (!take(j)) continue;
        const double* src = A + (size_t)j * m;
        for (int i = 0; i < m; ++i) b1[i] = std::fma(-src[i], w[j], b1[i]);
    }
}

// The rule's selector (its LDS checked and opted in) and the bound state beside the tableau of p: U (cols entries), the
// flags (up null: none set), the flip counter, the dual selector's scratch and, under LP_PIVOT_DEVEX, the weights
// (run_bounded_phase sets them; under LP_DUAL_DEVEX the dual loop's m weights live in the same cols >= m entries).
// buf must be freed before the problem (hipFree waits for the queued kernels).
int bounded_large_state(lp_simplex_problem* p, lp_device_buffer& buf, BoundedLargeDev& bd, const double* U,
                        const int* up, int cols, int rule, int dual_rule = LP_DUAL_DANTZIG) {
    lp_context* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    const int rc = lp_bounded_large_prepare(p, rule);
    if (rc) return rc;
    LP_HIP(ctx, lp_carve_malloc(&buf.ptr, [&](lp_carver& cv) {
        bd.U = cv.take<double>(sizeof(double) * (size_t)cols);
        bd.q = cv.take<double>(sizeof(double) * (size_t)p->dev.ld);
        bd.w = rule == LP_PIVOT_DEVEX || dual_rule == LP_DUAL_DEVEX ? cv.take<double>(sizeof(double) * (size_t)cols) : nullptr;
        bd.up = cv.take<int>(sizeof(int) * (size_t)cols);
        bd.flips = cv.take<int>(sizeof(int));
    }));
    LP_HIP(ctx, hipMemcpyAsync(bd.U, U, sizeof(double) * (size_t)cols, hipMemcpyHostToDevice, s));
    if (up)
        LP_HIP(ctx, hipMemcpyAsync(bd.up, up, sizeof(int) * (size_t)cols, hipMemcpyHostToDevice, s));
    else
        LP_HIP(ctx, hipMemsetAsync(bd.up, 0, sizeof(int) * (size_t)cols, s));
    LP_HIP(ctx, hipMemsetAsync(bd.flips, 0, sizeof(int), s));
    return LP_OPTIMAL;
}

// One loop on the tableau of p: the bounded selector + rank-1 update pair per iteration, polled by lp_poll_pivots.
// *iters = its pivots plus flips, *flips = the flips since the start of the solve.  rule: the primal selector (Devex:
// the weights are reset on the stream first).  dual: the dual selector of dual_rule in its place (lp_bounded_dual_prepare
// has run for it; LP_DUAL_DEVEX: its m weights are reset on the stream first) under dual_ratio (LP_DUAL_RATIO_LONG_STEP:
// the dual loop flips too, and *iters stays its pivots alone).
int run_bounded_phase(lp_simplex_problem* p, const BoundedLargeDev& bd, int rule, double eps, int max_iter, int* iters,
                      int* flips, bool dual = false, int dual_rule = LP_DUAL_DANTZIG,
                      int dual_ratio = LP_DUAL_RATIO_TEXTBOOK) {
    lp_context* ctx = p->ctx;
    lp_launch_begin(p, eps, max_iter);
    if (!dual && rule == LP_PIVOT_DEVEX) lp_bounded_large_reset_weights(p, bd);
    if (dual && dual_rule == LP_DUAL_DEVEX) lp_bounded_large_reset_weights(p, bd, true);
    int rc = lp_poll_pivots(p, [&](int batch) { return lp_bounded_large_queue(p, bd, batch, rule, dual, dual_rule, dual_ratio); });
    if (rc) return rc;
    rc = lp_download(ctx, "lp_simplex_bounded_large", {{flips, bd.flips, sizeof(int)}});
    if (rc) return rc;
    LP_HIP(ctx, hipGetLastError());
    *iters = p->h_state->iters;
    return p->h_state->status;
}

// Steps 5 and 6 of bounded_resolve_ref.c on an installed start: a classification launch, then the primal loop when
// every basic variable is within its bounds, else the dual loop when the start is dual feasible, else LP_BAD_ARG under
// who's name.  Returns the loop's status or a negative HIP error; count[0..2] += its dual pivots, primal pivots and
// flips.  prepare_dual: opt the dual selector's LDS in on the dual branch (the re-solve; the search did it up front).
// dual_rule: the pricing of the dual loop (the search passes none: Dantzig's).  dual_ratio: its ratio test (the search
// passes none: the textbook one); under LP_DUAL_RATIO_LONG_STEP the dual loop's flips are counted in count[2] too.
int bounded_run_from_start(lp_simplex_problem* p, const BoundedLargeDev& bd, const char* who, int rule, double eps,
                           int max_iter, bool prepare_dual, int* count, int dual_rule = LP_DUAL_DANTZIG,
                           int dual_ratio = LP_DUAL_RATIO_TEXTBOOK) {
    int flags = 0, iters = 0, flips = 0;
    int rc = lp_bounded_large_classify(p, bd, eps, &flags);
    if (rc) return rc;
    const bool dual = flags & 1;
    if (dual && (flags & 2)) LP_FAIL(p->ctx, LP_BAD_ARG, std::string(who) + ": the basis is neither primal nor dual feasible");
    if (dual && prepare_dual && (rc = lp_bounded_dual_prepare(p, dual_rule, dual_ratio)) != LP_OPTIMAL) return rc;
    rc = run_bounded_phase(p, bd, rule, eps, max_iter, &iters, &flips, dual, dual_rule, dual_ratio);
    if (rc < 0) return rc;
    count[dual ? 0 : 1] += dual ? iters : iters - flips;
    // (flips counts since the start of the solve, and the search runs textbook dual loops after primal ones on one
    // bound state: only a loop that flips may add it, or the primal loop's flips would be counted again)
    if (!dual || dual_ratio == LP_DUAL_RATIO_LONG_STEP) count[2] += flips;
    return rc;
}

// Step 9 of bounded_ref.c: for LP_OPTIMAL un-complement and un-shift v (n values, overwritten), the objective in index
// order, x_out (n_orig) and *obj_out; the basis and the flags for every status.
void bounded_large_outputs(int rc, int m, int n, int n_orig, const double* c, const double* lo, const double* U,
                           const int* up, const int* N, double* v, double* x_out, int* basis_out, int* at_upper_out,
                           double* obj_out) {
    if (rc == LP_OPTIMAL) {
        for (int j = 0; j < n; ++j) {
            const double w = up[j] ? U[j] - v[j] : v[j];
            v[j] = lo[j] == 0.0 ? w : lo[j] + w;
        }
        double z = 0.0;
        for (int j = 0; j < n; ++j) z += c[j] * v[j];
        for (int j = 0; j < n_orig; ++j) x_out[j] = v[j];
        *obj_out = z;
    }
    std::memcpy(basis_out, N, sizeof(int) * (size_t)m);
    for (int j = 0; j < n; ++j) at_upper_out[j] = up[j];
}

// ---- the pieces of lp_mip_bounded_solve_large.  What lives for one call: the pinned result, the problem record, one
// device allocation (A, b, c and the mask, the bound state, the node's lo and vertex, the incumbent, the records' bases
// and flags), the snapshot slots (one allocation each, made when the search first writes the slot) and what an install
// needs of the arguments.
struct MipLargeCall {
    struct Pinned {
        MipLargeResult* ptr = nullptr;
        ~Pinned() { (void)hipHostFree(ptr); }
    } pinned;   // (declared first: freed after the device buffers, whose hipFree waits for the queued kernels)
    ProblemOwner owner{nullptr, lp_simplex_free};
    lp_device_buffer buf;   // (freed before the problem on every return path)
    std::vector<lp_device_buffer> slots;   // the ring of lp_mip_bounded_solve_large_ex (freed before buf)
    std::vector<int> slot_level;           // the level a slot belongs to, -1: none
    BoundedLargeDev bd{};
    MipLargeDev md{};
    const double *A = nullptr, *c = nullptr;   // the caller's: the identity scan of an install reads them
    double eps = 0.0;
    int max_iter = 0;
    int dual_ratio = LP_DUAL_RATIO_TEXTBOOK;   // the ratio test of every dual loop of the search
};

// Step 2 of the reference on a node's bounds, basis and flags: its status or a negative HIP error, stats[1..3] counted.
int mip_large_install(MipLargeCall& k, const char* who, const double* lov, const double* hiv, const int* N,
                      const int* up, int* stats) {
    lp_simplex_problem* p = k.owner.get();
    lp_context* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    const int m = p->dev.m, n = p->dev.n;
    for (int j = 0; j < n; ++j)
        if (hiv[j] < lov[j]) return LP_INFEASIBLE;
    std::vector<double> U((size_t)n);
    for (int j = 0; j < n; ++j) U[(size_t)j] = hiv[j] - lov[j];
    LP_HIP(ctx, hipMemcpyAsync(k.md.lo, lov, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(k.bd.U, U.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(k.bd.up, up, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemsetAsync(k.bd.flips, 0, sizeof(int), s));
    lp_mip_large_stage(p, k.bd, k.md);
    // the unit columns in order with zero costs: the m basic columns and their signs, O(m^2) on the host
    bool identity, zero_costs;
    lp_slack_identity(k.A, m, k.c, N, &identity, &zero_costs, up);
    const int r = lp_simplex_install(p, N, identity, zero_costs);
    if (r) return r;
    if (p->init_status != LP_OPTIMAL) return p->init_status;   // LP_SINGULAR
    return bounded_run_from_start(p, k.bd, who, LP_PIVOT_DANTZIG, k.eps, k.max_iter, false, stats + 1, LP_DUAL_DANTZIG,
                                  k.dual_ratio);
}

// One branching: the column, its value, the node's objective, which child went first, whether the second was taken
struct MipRecord {
    int j, first_down, second_taken;
    double v, z;
};

bool mip_beats(int maximize, double z, double zs, double g) { return maximize ? (z > zs + g) : (z < zs - g); }

// The dual loop of a first child or of a restored second child, where the tableau stands: its status or a negative HIP
// error, stats[1] += its pivots.  Under LP_DUAL_RATIO_LONG_STEP the loop flips too: bd.flips counts since the last
// install's memset (bounded_run_from_start relies on that for the install's own loop), so it is zeroed on the stream
// ahead of the loop and stats[3] += this loop's flips alone, whatever ran since that install.  The textbook loop
// queues what it always queued.
int mip_large_child_loop(MipLargeCall& k, int* stats) {
    lp_simplex_problem* p = k.owner.get();
    const bool flipping = k.dual_ratio == LP_DUAL_RATIO_LONG_STEP;
    if (flipping) LP_HIP(p->ctx, hipMemsetAsync(k.bd.flips, 0, sizeof(int), p->ctx->stream));
    int iters = 0, flips = 0;
    const int st = run_bounded_phase(p, k.bd, LP_PIVOT_DANTZIG, k.eps, k.max_iter, &iters, &flips, true, LP_DUAL_DANTZIG,
                                     k.dual_ratio);
    if (st < 0) return st;
    stats[1] += iters;
    if (flipping) stats[3] += flips;
    return st;
}

// Step 8 of the reference: the status and, where one is defined (*bound is left alone otherwise), the bound.  Open are
// the abandoned nodes (have_ab, zab), the records whose second child was not taken and, after a stop, the one on top.
int mip_large_verdict(const std::vector<MipRecord>& rec, int top, int stop, int found, int have_ab, double zab,
                      double zstar, double gap, int maximize, double* bound) {
    int have_open = have_ab;
    double zo = zab;
    for (int k = 0; k <= top; ++k)
        if (!rec[(size_t)k].second_taken || (stop != LP_OPTIMAL && k == top)) {
            if (!have_open || mip_beats(maximize, rec[(size_t)k].z, zo, 0.0)) zo = rec[(size_t)k].z;
            have_open = 1;
        }
    if (found) *bound = (have_open && mip_beats(maximize, zo, zstar, gap)) ? zo : zstar;
    else if (have_open) *bound = zo;
    if (stop != LP_OPTIMAL) return stop;
    if (found) return (have_ab && mip_beats(maximize, zab, zstar, gap)) ? LP_ITER_LIMIT : LP_OPTIMAL;
    return have_ab ? LP_ITER_LIMIT : LP_INFEASIBLE;
}

// Depth-first branch-and-bound over the bounds on the HBM tableau (tests/ref/mip_bounded_ref.c is the definition; the
// kernels are mip_bounded_large.hip's).  The host drives the search and keeps what is O(depth): j, v, z and the sides of
// the records, the incumbent's objective, the counters.  A, b and c go up once; the tableau, the bound state, the node's
// lo, the incumbent and the records' bases and flags stay on the device.  A node that ended LP_OPTIMAL costs one launch
// of the node kernel and one sync; its first child continues on the live tableau with the bounded dual loop (no crash);
// a second child is staged on the device from the persistent A and installed by lp_simplex_install.
// With snapshots = K > 0 (tests/ref/mip_bounded_snapshots_ref.c): a node that branches at level L and dives is saved, as
// it stood before the dive's bound change, in slot L mod K' (K' = min(K, max_depth): L < max_depth, so the slot and
// whether it survives are those of L mod K); a second child whose slot still belongs to its level is restored from it
// and continues like a first child, with one sync for its bound change and none of the rebuild's work.
// stats_out: nstats entries, 5 (the counters of the reference) or 7 (then the second children restored and rebuilt).
// dual_ratio (tests/ref/mip_bounded_long_step_ref.c): the ratio test of every dual loop, the install's, a first
// child's and a restored second child's; under LP_DUAL_RATIO_LONG_STEP stats[3] counts their flips too.  A snapshot is
// queued before the child's loop and the flags of a restored node come from the level's record, which the node kernel
// wrote before the bound change, so the flips of a child's loop are in neither.
int mip_large_search(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo,
                     const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig,
                     const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes,
                     int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out,
                     int nstats, int snapshots, int dual_ratio) {
    const char* who = "lp_mip_bounded_solve_large";
    const bool any_null = !x_out || !obj_out || !bound_out || !found_out || !stats_out || !A || !b || !c || !lo || !hi ||
                          !basis_in || !at_upper_in || !integer;
    // step 1: the entry and the start as the re-solve, the search's own arguments, integral bounds on the marked columns
    int rc = check_bounded_entry(ctx, who, LP_PIVOT_DANTZIG, any_null, eps, m, n, n_orig, lo, hi);
    if (rc) return rc;
    rc = check_bounded_start(ctx, who, n, m, hi, basis_in, at_upper_in);
    if (rc) return rc;
    rc = lp_mip_check_search(ctx, who, n, n_orig, integer, int_tol, gap, max_depth, LP_MIP_BOUNDED_MAX_DEPTH, max_nodes);
    if (rc) return rc;
    for (int j = 0; j < n_orig; ++j)
        if (integer[j] && (lo[j] != std::floor(lo[j]) || (std::isfinite(hi[j]) && hi[j] != std::floor(hi[j]))))
            LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": an integer column has a fractional bound");
    // ---- the problem record, the selectors' LDS (m <= 9960), the call's allocations and the four uploads (queued)
    MipLargeCall k;
    lp_simplex_problem* p = nullptr;
    rc = lp_simplex_alloc(ctx, m, n, nullptr, maximize, n, &p);
    if (rc) return rc;
    k.owner.reset(p);
    rc = lp_bounded_large_prepare(p, LP_PIVOT_DANTZIG);
    if (rc) return rc;
    rc = lp_bounded_dual_prepare(p, LP_DUAL_DANTZIG, dual_ratio);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    BoundedLargeDev& bd = k.bd;
    MipLargeDev& md = k.md;
    double *dA = nullptr, *db = nullptr, *dc = nullptr;   // (md's own pointers to them are const)
    int* dmask = nullptr;
    LP_HIP(ctx, lp_carve_malloc(&k.buf.ptr, [&](lp_carver& cv) {
        dA = cv.take<double>(sizeof(double) * (size_t)m * n);
        db = cv.take<double>(sizeof(double) * (size_t)m);
        dc = cv.take<double>(sizeof(double) * (size_t)n);
        bd.U = cv.take<double>(sizeof(double) * (size_t)n);
        bd.q = cv.take<double>(sizeof(double) * (size_t)p->dev.ld);
        md.lo = cv.take<double>(sizeof(double) * (size_t)n);
        md.x = cv.take<double>(sizeof(double) * (size_t)n);
        md.xinc = cv.take<double>(sizeof(double) * (size_t)n_orig);
        bd.up = cv.take<int>(sizeof(int) * (size_t)n);
        bd.flips = cv.take<int>(sizeof(int));
        dmask = cv.take<int>(sizeof(int) * (size_t)n);
        md.rec_basis = cv.take<int>(sizeof(int) * (size_t)max_depth * m);
        md.rec_up = cv.take<int>(sizeof(int) * (size_t)max_depth * n);
    }));
    LP_HIP(ctx, hipHostMalloc(&k.pinned.ptr, sizeof(MipLargeResult)));
    md.A = dA; md.b = db; md.c = dc; md.integer = dmask; md.result = k.pinned.ptr;
    md.n_orig = n_orig; md.max_depth = max_depth; md.int_tol = int_tol; md.gap = gap;
    LP_HIP(ctx, hipMemcpyAsync(dA, A, sizeof(double) * (size_t)m * n, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(db, b, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(dc, c, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(dmask, integer, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    k.A = A; k.c = c; k.eps = eps; k.max_iter = max_iter; k.dual_ratio = dual_ratio;
    const int K = std::min(snapshots, max_depth);
    const size_t slot_bytes = lp_mip_large_slot_bytes(m, n);
    k.slots = std::vector<lp_device_buffer>((size_t)K);
    k.slot_level.assign((size_t)K, -1);

    int stats[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < n_orig; ++j) x_out[j] = NAN;
    *obj_out = NAN;
    *bound_out = NAN;
    *found_out = 0;

    std::vector<MipRecord> rec((size_t)max_depth);
    std::vector<double> lov((size_t)n), hiv((size_t)n);
    std::vector<int> N((size_t)m), up((size_t)n);

    // ---- root
    int st = mip_large_install(k, who, lo, hi, basis_in, at_upper_in, stats);
    if (st < 0) return st;
    stats[0] = 1;
    int status = st;
    if (st != LP_OPTIMAL) {
        if (st == LP_UNBOUNDED || st == LP_ITER_LIMIT) *bound_out = maximize ? INFINITY : -INFINITY;
    } else {
        int L = 0, top = -1, found = 0, stop = LP_OPTIMAL, have_ab = 0;
        double zstar = 0.0, zab = 0.0;
        for (;;) {
            bool backtrack = true;
            if (st == LP_OPTIMAL) {
                // steps 3 to 5 on the device; a node is counted before it starts, so the dive waits for the budget
                const int dive = stats[0] < max_nodes;
                lp_mip_large_node(p, bd, md, L, found, zstar, dive);
                LP_HIP(ctx, hipStreamSynchronize(s));
                LP_HIP(ctx, hipGetLastError());
                const MipLargeResult r = *k.pinned.ptr;
                if (r.what == LP_MIPL_INTEGRAL) {
                    found = 1;
                    zstar = r.z;
                } else if (r.what == LP_MIPL_ABANDONED) {
                    if (!have_ab || mip_beats(maximize, r.z, zab, 0.0)) zab = r.z;
                    have_ab = 1;
                } else if (r.what == LP_MIPL_BRANCHED || r.what == LP_MIPL_NOT_BASIC) {
                    rec[(size_t)L] = MipRecord{r.j, (r.v - std::floor(r.v)) <= 0.5, 0, r.v, r.z};
                    top = L;
                    if (!dive) { stop = LP_ITER_LIMIT; break; }
                    if (r.what == LP_MIPL_NOT_BASIC) { stop = LP_BAD_ARG; break; }
                    if (K > 0) {   // step 4': the node as it stood before the bound change, into slot L mod K
                        lp_device_buffer& slot = k.slots[(size_t)(L % K)];
                        if (!slot.ptr) {
                            const hipError_t e = hipMalloc(&slot.ptr, slot_bytes);
                            if (e != hipSuccess) {
                                (void)hipGetLastError();
                                LP_FAIL(ctx, -(int)e, std::string(who) + ": a snapshot slot: " + hipGetErrorString(e));
                            }
                        }
                        k.slot_level[(size_t)(L % K)] = L;
                        lp_mip_large_save(p, bd, md, slot.ptr, r);
                    }
                    ++L;
                    ++stats[0];
                    if (L > stats[4]) stats[4] = L;
                    if (r.un_negative) {
                        st = LP_INFEASIBLE;   // without a pivot
                    } else {
                        st = mip_large_child_loop(k, stats);
                        if (st < 0) return st;
                    }
                    backtrack = false;
                }
            } else if (st != LP_INFEASIBLE) {
                stop = st;
                break;
            }
            if (!backtrack) continue;
            while (top >= 0 && rec[(size_t)top].second_taken) --top;
            if (top < 0) break;
            rec[(size_t)top].second_taken = 1;
            if (stats[0] >= max_nodes) { stop = LP_ITER_LIMIT; break; }
            L = top + 1;
            if (K > 0 && k.slot_level[(size_t)(top % K)] == top) {
                // ---- step 6': the second child from the snapshot of its level, the other side
                const MipRecord& R = rec[(size_t)top];
                k.slot_level[(size_t)(top % K)] = -1;
                ++stats[0];
                ++stats[5];
                if (L > stats[4]) stats[4] = L;
                lp_mip_large_second_child(p, bd, md, k.slots[(size_t)(top % K)].ptr, top, R.j, R.v, !R.first_down);
                LP_HIP(ctx, hipStreamSynchronize(s));
                LP_HIP(ctx, hipGetLastError());
                const MipLargeResult r = *k.pinned.ptr;
                if (r.what == LP_MIPL_NOT_BASIC) { stop = LP_BAD_ARG; break; }
                if (r.un_negative) {
                    st = LP_INFEASIBLE;   // without a pivot
                } else {
                    st = mip_large_child_loop(k, stats);
                    if (st < 0) return st;
                }
                continue;
            }
            // ---- the second child of record `top`: the root's bounds overlaid in level order, the recorded start
            ++stats[6];
            std::memcpy(lov.data(), lo, sizeof(double) * (size_t)n);
            std::memcpy(hiv.data(), hi, sizeof(double) * (size_t)n);
            for (int l = 0; l < L; ++l) {
                const MipRecord& R = rec[(size_t)l];
                const int down = R.second_taken ? !R.first_down : R.first_down;
                if (down) hiv[(size_t)R.j] = std::floor(R.v);
                else lov[(size_t)R.j] = std::ceil(R.v);
            }
            rc = lp_download(ctx, who, {{N.data(), md.rec_basis + (size_t)top * m, sizeof(int) * (size_t)m},
                                        {up.data(), md.rec_up + (size_t)top * n, sizeof(int) * (size_t)n}});
            if (rc) return rc;
            ++stats[0];
            if (L > stats[4]) stats[4] = L;
            st = mip_large_install(k, who, lov.data(), hiv.data(), N.data(), up.data(), stats);
            if (st < 0) return st;
        }
        // ---- status and bound (step 8)
        double bound = NAN;
        status = mip_large_verdict(rec, top, stop, found, have_ab, zab, zstar, gap, maximize, &bound);
        if (found) {
            rc = lp_download(ctx, who, {{x_out, md.xinc, sizeof(double) * (size_t)n_orig}});
            if (rc) return rc;
            *found_out = 1;
            *obj_out = zstar;
        }
        *bound_out = bound;
    }
    std::memcpy(stats_out, stats, sizeof(int) * (size_t)nstats);
    if (status == LP_BAD_ARG) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": the basis is neither primal nor dual feasible");
    if (status == LP_SINGULAR) ctx->last_error = std::string(who) + ": the basis matrix is singular";
    return status;
}

}  // namespace

extern "C" {

// The bounded-variable two-phase simplex on the HBM tableau (tests/ref/bounded_ref.c is the definition): the flow of
// lp_simplex_two_phase_ex with the selector of simplex_bounded_launch.hip in both phases.  The set-up arithmetic
// (shift, sign changes, U, the phase-II costs of complemented columns, the outputs) runs here on the host in the
// reference's order; every pivot and flip runs on the GPU.
int lp_simplex_bounded_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                             const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter,
                             double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out) {
    return lp_simplex_bounded_large_ex(ctx, A, m, n, b, c, lo, hi, maximize, n_orig, eps, max_iter, x_out, basis_out,
                                       at_upper_out, obj_out, iters_out, LP_PIVOT_DANTZIG);
}

// The same under a pivot rule (tests/ref/bounded_rules_ref.c): the rule picks the selector of both phases' loops; the
// drive-out, the phase-II costs and the outputs do not depend on it.
int lp_simplex_bounded_large_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter,
                                double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out,
                                int pivot_rule) {
    const char* who = "lp_simplex_bounded_large";
    const bool any_null = !x_out || !basis_out || !at_upper_out || !obj_out || !iters_out || !A || !b || !c || !lo || !hi;
    int rc = check_bounded_entry(ctx, who, pivot_rule, any_null, eps, m, n, n_orig, lo, hi);
    if (rc) return rc;
    const int na = n + m;
    int it[4] = {0, 0, 0, 0};
    for (int t = 0; t < m; ++t) basis_out[t] = n + t;
    for (int j = 0; j < n; ++j) at_upper_out[j] = 0;
    std::memcpy(iters_out, it, sizeof(it));
    rc = check_crossed(ctx, who, lo, hi, n);
    if (rc) return rc;

    // shift x = lo + x' (b' accumulated in ascending j, lo_j == 0 skipped), U = hi - lo, then make_b_nonneg and
    // createAuxiliaryProblem on [A | b'] as lp_simplex_two_phase_ex
    std::vector<double> A1((size_t)m * na, 0.0), b1((size_t)m), c1((size_t)na, 0.0), xa((size_t)na), U((size_t)na);
    std::vector<int> N((size_t)m), up((size_t)na, 0);
    for (int j = 0; j < n; ++j) U[(size_t)j] = hi[j] - lo[j];
    for (int k = n; k < na; ++k) U[(size_t)k] = INFINITY;
    for (int i = 0; i < m; ++i) b1[(size_t)i] = b[i];
    shift_rhs(A, m, n, lo, [&](int j) { return lo[j] != 0.0; }, b1.data());
    auxiliary_problem(A, m, n, b1.data(), eps, A1.data(), b1.data(), c1.data(), N.data());

    lp_simplex_problem* p = nullptr;
    rc = lp_simplex_upload(ctx, A1.data(), m, na, b1.data(), c1.data(), N.data(), 0, na, &p);
    if (rc) return rc;
    ProblemOwner owner(p, lp_simplex_free);
    // the bound state beside the tableau (buf is freed before the problem on every return path)
    hipStream_t s = ctx->stream;
    lp_device_buffer buf;
    BoundedLargeDev bd{};
    rc = bounded_large_state(p, buf, bd, U.data(), nullptr, na, pivot_rule);
    if (rc) return rc;
    auto download_flags = [&]() { return lp_download(ctx, who, {{up.data(), bd.up, sizeof(int) * (size_t)n}}); };

    // ---- phase I: minimise the sum of the artificials
    int iters = 0, flips1 = 0, flips = 0;
    rc = run_bounded_phase(p, bd, pivot_rule, eps, max_iter, &iters, &flips1);
    if (rc < 0) return rc;
    it[0] = iters - flips1;
    it[3] = flips1;
    if (rc == LP_OPTIMAL) rc = lp_simplex_download(p, xa.data(), N.data(), nullptr, nullptr, nullptr, 0, nullptr);
    if (rc == LP_OPTIMAL) rc = phase1_verdict(ctx, who, xa.data(), m, n, eps);
    if (rc == LP_OPTIMAL) rc = drive_out_artificials(p, who, N.data(), m, n, eps, &it[1]);
    if (rc >= 0) {
        const int rf = download_flags();
        if (rf) rc = rf;
    }
    // ---- phase II on the phase-I tableau: a complemented column's cost changes sign
    if (rc == LP_OPTIMAL) {
        std::vector<double> c2((size_t)n);
        for (int j = 0; j < n; ++j) c2[(size_t)j] = up[(size_t)j] ? -c[j] : c[j];
        rc = lp_simplex_phase2_costs(p, c2.data(), n, maximize, n);   // (n_orig = n: the download below returns every v_j)
    }
    if (rc == LP_OPTIMAL) {
        rc = run_bounded_phase(p, bd, pivot_rule, eps, max_iter, &iters, &flips);
        if (rc >= 0) {
            it[2] = iters - (flips - flips1);
            it[3] = flips;
            int rd = rc == LP_OPTIMAL ? lp_simplex_download(p, xa.data(), N.data(), nullptr, nullptr, nullptr, 0, nullptr)
                                      : download_basis(p, N.data());
            if (rd == LP_OPTIMAL) rd = download_flags();
            if (rd) rc = rd;
        }
    } else if (rc > 0) {
        const int rd = download_basis(p, N.data());
        if (rd) rc = rd;
    }
    (void)hipStreamSynchronize(s);
    if (rc < 0) return rc;
    bounded_large_outputs(rc, m, n, n_orig, c, lo, U.data(), up.data(), N.data(), xa.data(), x_out, basis_out,
                          at_upper_out, obj_out);
    std::memcpy(iters_out, it, sizeof(it));
    return rc;
}

// The re-solve of a bounded LP from a basis and flags on the HBM tableau (tests/ref/bounded_resolve_ref.c is the
// definition): the checks and the set-up arithmetic (shift, the flagged columns held complemented) run here on the
// host in the reference's order, lp_simplex_upload installs the basis on the (m+1) x (n+1) tableau (no artificial
// columns), a classification launch picks the loop, and every pivot and flip runs on the GPU: the primal loop is
// lp_simplex_bounded_large's phase II, the dual loop the selector k_simplex_select_dual_bounded.
int lp_simplex_bounded_resolve_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                     const double* lo, const double* hi, const int* basis_in, const int* at_upper_in,
                                     int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out,
                                     int* at_upper_out, double* obj_out, int* iters_out) {
    return lp_simplex_bounded_resolve_large_ex(ctx, A, m, n, b, c, lo, hi, basis_in, at_upper_in, maximize, n_orig, eps,
                                               max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out,
                                               LP_PIVOT_DANTZIG);
}

// The same under a pivot rule (tests/ref/bounded_resolve_rules_ref.c): the rule governs the primal loop only; the
// crash, the classification and the dual loop are the same under every rule.
int lp_simplex_bounded_resolve_large_ex(lp_context* ctx, const double* A, int m, int n, const double* b,
                                        const double* c, const double* lo, const double* hi, const int* basis_in,
                                        const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter,
                                        double* x_out, int* basis_out, int* at_upper_out, double* obj_out,
                                        int* iters_out, int pivot_rule) {
    return lp_simplex_bounded_resolve_large_dual_ex(ctx, A, m, n, b, c, lo, hi, basis_in, at_upper_in, maximize, n_orig,
                                                    eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out,
                                                    pivot_rule, LP_DUAL_DANTZIG);
}

// The same under a dual pricing rule too (tests/ref/bounded_resolve_dual_rules_ref.c): dual_rule picks the dual loop's
// selector and nothing else; under LP_DUAL_DANTZIG every launch is lp_simplex_bounded_resolve_large_ex's.
int lp_simplex_bounded_resolve_large_dual_ex(lp_context* ctx, const double* A, int m, int n, const double* b,
                                             const double* c, const double* lo, const double* hi, const int* basis_in,
                                             const int* at_upper_in, int maximize, int n_orig, double eps,
                                             int max_iter, double* x_out, int* basis_out, int* at_upper_out,
                                             double* obj_out, int* iters_out, int pivot_rule, int dual_rule) {
    return lp_simplex_bounded_resolve_large_ratio_ex(ctx, A, m, n, b, c, lo, hi, basis_in, at_upper_in, maximize, n_orig,
                                                     eps, max_iter, x_out, basis_out, at_upper_out, obj_out, iters_out,
                                                     pivot_rule, dual_rule, LP_DUAL_RATIO_TEXTBOOK);
}

// The same with a choice of the dual loop's ratio test too (tests/ref/bounded_resolve_long_step_ref.c): dual_ratio picks
// the textbook or the bound-flipping form of the dual selector and nothing else; under LP_DUAL_RATIO_TEXTBOOK every
// launch is lp_simplex_bounded_resolve_large_dual_ex's.  iters_out[2] counts the dual loop's flips too.
int lp_simplex_bounded_resolve_large_ratio_ex(lp_context* ctx, const double* A, int m, int n, const double* b,
                                              const double* c, const double* lo, const double* hi, const int* basis_in,
                                              const int* at_upper_in, int maximize, int n_orig, double eps,
                                              int max_iter, double* x_out, int* basis_out, int* at_upper_out,
                                              double* obj_out, int* iters_out, int pivot_rule, int dual_rule,
                                              int dual_ratio) {
    const char* who = "lp_simplex_bounded_resolve_large";
    const bool any_null = !x_out || !basis_out || !at_upper_out || !obj_out || !iters_out || !A || !b || !c || !lo ||
                          !hi || !basis_in || !at_upper_in;
    if (!ctx) return LP_BAD_ARG;
    if (!lp_dual_ratio_known(dual_ratio)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": unknown dual ratio test");
    if (!lp_dual_rule_known(dual_rule)) LP_FAIL(ctx, LP_BAD_ARG, std::string(who) + ": unknown dual rule");
    int rc = check_bounded_entry(ctx, who, pivot_rule, any_null, eps, m, n, n_orig, lo, hi);
    if (rc) return rc;
    rc = check_bounded_start(ctx, who, n, m, hi, basis_in, at_upper_in);
    if (rc) return rc;
    int it[3] = {0, 0, 0};
    std::vector<int> N(basis_in, basis_in + m), up(at_upper_in, at_upper_in + n);   // (the outputs may be the inputs)
    std::memcpy(basis_out, N.data(), sizeof(int) * (size_t)m);
    std::memcpy(at_upper_out, up.data(), sizeof(int) * (size_t)n);
    std::memcpy(iters_out, it, sizeof(it));
    rc = check_crossed(ctx, who, lo, hi, n);
    if (rc) return rc;

    // steps 2 and 3 of the reference: shift x = lo + x', U = hi - lo, the chain goes on over the flagged columns with
    // U_j; those columns and their costs change sign
    std::vector<double> A1(A, A + (size_t)m * n), b1(b, b + m), c1(c, c + n), xa((size_t)n), U((size_t)n);
    for (int j = 0; j < n; ++j) U[(size_t)j] = hi[j] - lo[j];
    shift_rhs(A, m, n, lo, [&](int j) { return lo[j] != 0.0; }, b1.data());
    shift_rhs(A, m, n, U.data(), [&](int j) { return up[(size_t)j] != 0; }, b1.data());
    for (int j = 0; j < n; ++j) {
        if (!up[(size_t)j]) continue;
        double* col = A1.data() + (size_t)j * m;
        for (int i = 0; i < m; ++i) col[i] = -col[i];
        c1[(size_t)j] = -c1[(size_t)j];
    }
    // step 4: the basis install (n_orig = n: the download below returns every column's value)
    lp_simplex_problem* p = nullptr;
    rc = lp_simplex_upload(ctx, A1.data(), m, n, b1.data(), c1.data(), N.data(), maximize, n, &p);
    if (rc) return rc;
    ProblemOwner owner(p, lp_simplex_free);
    if (p->init_status != LP_OPTIMAL)   // LP_SINGULAR: the given basis and flags stay in the outputs
        LP_FAIL(ctx, p->init_status, std::string(who) + ": the basis matrix is singular");
    lp_device_buffer buf;   // (freed before the problem on every return path)
    BoundedLargeDev bd{};
    rc = bounded_large_state(p, buf, bd, U.data(), up.data(), n, pivot_rule, dual_rule);
    if (rc) return rc;
    // steps 5 and 6: the loop the start allows (a refusal or a HIP error leaves iters_out at zero)
    rc = bounded_run_from_start(p, bd, who, pivot_rule, eps, max_iter, true, it, dual_rule, dual_ratio);
    if (rc < 0 || rc == LP_BAD_ARG) return rc;
    int rd = rc == LP_OPTIMAL ? lp_simplex_download(p, xa.data(), N.data(), nullptr, nullptr, nullptr, 0, nullptr)
                              : download_basis(p, N.data());
    if (rd == LP_OPTIMAL) rd = lp_download(ctx, who, {{up.data(), bd.up, sizeof(int) * (size_t)n}});
    if (rd) return rd;
    bounded_large_outputs(rc, m, n, n_orig, c, lo, U.data(), up.data(), N.data(), xa.data(), x_out, basis_out,
                          at_upper_out, obj_out);
    std::memcpy(iters_out, it, sizeof(it));
    return rc;
}

// The search beyond LDS (mip_large_search above): the definition is tests/ref/mip_bounded_ref.c.
int lp_mip_bounded_solve_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                               const double* lo, const double* hi, const int* basis_in, const int* at_upper_in,
                               int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap,
                               int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out,
                               double* bound_out, int* found_out, int* stats_out) {
    return mip_large_search(ctx, A, m, n, b, c, lo, hi, basis_in, at_upper_in, maximize, n_orig, integer, eps, int_tol,
                            gap, max_depth, max_nodes, max_iter, x_out, obj_out, bound_out, found_out, stats_out, 5, 0,
                            LP_DUAL_RATIO_TEXTBOOK);
}

// The same with up to `snapshots` tableau snapshots (tests/ref/mip_bounded_snapshots_ref.c): 0 launches what the entry
// above launches.
int lp_mip_bounded_solve_large_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                  const double* lo, const double* hi, const int* basis_in, const int* at_upper_in,
                                  int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap,
                                  int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out,
                                  double* bound_out, int* found_out, int* stats_out, int snapshots) {
    return lp_mip_bounded_solve_large_ratio_ex(ctx, A, m, n, b, c, lo, hi, basis_in, at_upper_in, maximize, n_orig,
                                               integer, eps, int_tol, gap, max_depth, max_nodes, max_iter, x_out, obj_out,
                                               bound_out, found_out, stats_out, snapshots, LP_DUAL_RATIO_TEXTBOOK);
}

// The same with a choice of the ratio test of the search's dual loops (tests/ref/mip_bounded_long_step_ref.c): an
// unknown dual_ratio is refused before anything else is looked at; LP_DUAL_RATIO_TEXTBOOK launches what the entry above
// launches, LP_DUAL_RATIO_LONG_STEP the selector k_simplex_select_dual_bounded_long in every dual loop.
int lp_mip_bounded_solve_large_ratio_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                                        const double* lo, const double* hi, const int* basis_in, const int* at_upper_in,
                                        int maximize, int n_orig, const int* integer, double eps, double int_tol,
                                        double gap, int max_depth, int max_nodes, int max_iter, double* x_out,
                                        double* obj_out, double* bound_out, int* found_out, int* stats_out,
                                        int snapshots, int dual_ratio) {
    if (!ctx) return LP_BAD_ARG;
    if (!lp_dual_ratio_known(dual_ratio))
        LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve_large: unknown dual ratio test");
    if (snapshots < 0 || snapshots > LP_MIP_BOUNDED_MAX_SNAPSHOTS)
        LP_FAIL(ctx, LP_BAD_ARG, "lp_mip_bounded_solve_large: snapshots outside [0, 1024]");
    return mip_large_search(ctx, A, m, n, b, c, lo, hi, basis_in, at_upper_in, maximize, n_orig, integer, eps, int_tol,
                            gap, max_depth, max_nodes, max_iter, x_out, obj_out, bound_out, found_out, stats_out, 7,
                            snapshots, dual_ratio);
}

// The device bytes `snapshots` slots take at m x n: each the (m+1) x ld tableau (ld = n + 1 rounded up to 8) and two
// vectors of n doubles rounded up to 2.  A host call.
int lp_mip_bounded_snapshot_bytes(int m, int n, int snapshots, unsigned long long* bytes_out) {
    if (!bytes_out || m <= 0 || n < m || snapshots < 0 || snapshots > LP_MIP_BOUNDED_MAX_SNAPSHOTS) return LP_BAD_ARG;
    *bytes_out = (unsigned long long)snapshots * (unsigned long long)lp_mip_large_slot_bytes(m, n);
    return LP_OPTIMAL;
}

}  // extern "C"
