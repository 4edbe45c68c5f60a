// simplex_problem.hpp — device-side state of one single-LP tableau solve.
#pragma once

#include <functional>
#include <memory>

#include "lp_internal.hpp"

struct SimplexState {
    int status;       // kRunning (-100) while pivoting, then an LP_* code
    int iters;        // pivots executed (the reference's `iteration`, SimplexSolover.h:427)
    int max_iter;     // MAX_ITER, :426
    int enter;        // entering column of the pending pivot
    int leave;        // leaving basis POSITION (= tableau row) of the pending pivot
    int pivot_valid;  // 1 if select staged a pivot for the update kernel
    int pad0, pad1;
    double eps;       // Solver::EPS, :13
    double minpiv, maxpiv;  // crash: smallest / largest |pivot|
};

// Everything the kernels need, passed by value.
struct SimplexDev {
    int m, n, ld;     // ld = padded row length of T (multiple of 8 doubles)
    int maximize;
    int trace_cap;
    double* T;        // (m+1) x ld row-major tableau
    double* lcol;     // m+1: eta column of F (:198-204); entry r holds 1/u_r
    double* prow;     // ld: copy of the pivot row before the update
    int* basis;       // m: N, basis by position (:419)
    unsigned char* nonbasic;  // n: complement(n, N) as flags (:97-108)
    unsigned char* rowused;   // m: crash bookkeeping
    int* rowpos;      // m: crash — tableau row chosen for basis position t
    int* trace_enter; // trace_cap
    int* trace_leave;
    SimplexState* state;
};

// Look-ahead batch buffers (simplex_lookahead.hip).
struct LookDev {
    int J;          // pivots staged per batch
    int rows_pad;   // row stride of etaL (m+1 rounded up to 8)
    double* etaL;   // J x rows_pad: eta columns of F (:198-204); entry r = 1/u_r, entry m = cost row
    double* etaP;   // J x ld: pivot rows before scaling (entry n = xB_r)
    double* dvec;   // ld: current reduced-cost row (entry n = -objective)
    double* rhs;    // rows_pad: current xB
    int* piv;       // 2 x J: (entering column, leaving position) of each staged pivot
    int* count;     // pivots staged by the last selector launch
    unsigned long long* stamps;  // diagnostic: 8 s_memtime stamps per pivot (nullptr = off)
};

// Chip-resident solve (simplex_resident.hip): the tableau lives in the registers of G co-resident
// workgroups (cpt columns each) for the whole solve; per pivot they exchange one 16-byte pricing record, 8-15
// slice records of the ratio test and one candidate column each through these buffers (8-byte {epoch tag, value}
// granules).
struct ResidentDev {
    int G;          // participating workgroups = ceil(n / columns per workgroup)
    int stride;     // participants are the blocks b with b % stride == 0 (8: one XCD under round-robin dispatch)
    int mpad;       // row threads per workgroup = m rounded up to 64 (one tableau row per thread)
    int cpt;        // tableau columns per workgroup: 32 (m <= 512) or 16 (m <= 960)
    int flags;      // bit 0: write-through stores even when all participants share an XCD; bit 1: injected failure (tests)
    char* comm;     // one allocation, zeroed before every launch; carved below (byte offsets)
    unsigned prec_off;           // [2][G] pricing records (16 bytes)
    unsigned srec_off;           // [2][G][2][16] slice records of the ratio test (A granules, B granules)
    unsigned col_off;            // [3][G][mpad] candidate columns
    unsigned dpub_off, recS_off, colS_off, census_off, abort_off, comm_bytes;
};

struct lp_simplex_problem {
    lp_context* ctx = nullptr;
    SimplexDev dev{};
    LookDev look{};
    ResidentDev res{};            // res.G == 0: shape outside the chip-resident path
    int n_orig = 0;
    size_t tableau_bytes = 0;
    void* arena = nullptr;        // ONE device allocation (from the context's pool) behind every pointer below
    size_t arena_bytes = 0;
    double* dT0 = nullptr;        // pristine initial tableau (after crash) for lp_simplex_reset; also the
                                  // staging area of the upload (column-major A) and of the crash's row permutation
    double* dscratchT = nullptr;  // scratch copy used by the update micro-benchmarks (allocated on first use)
    double* ov_T = nullptr;       // simplex_overlap.hip: the second tableau buffer, and the second eta slot
    double* ov_vec = nullptr;     // (pivot row, eta column, 8 ints); both allocated on first use
    double* dweights = nullptr;   // simplex_launch.hip: the n Devex weights (LP_PIVOT_DEVEX), allocated on first use
    int* dbasis0 = nullptr;
    unsigned char* dnonbasic0 = nullptr;
    double* dx = nullptr;         // n: extracted vertex
    SimplexState* h_state = nullptr;  // pinned
    std::vector<double> h_c;      // objective coefficients (Canonical::Evaluate on the host)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t res_ev0 = nullptr, res_ev1 = nullptr;   // around the chip-resident kernel launch
    std::vector<hipEvent_t> upd_events;  // 2 per timed rank-J update launch (look-ahead path)
    bool profile_updates = false;        // lp_simplex_profile: bracket update launches with events
    int init_status = LP_OPTIMAL; // LP_SINGULAR if the initial basis was singular
    int last_status = -100;
    int last_iters = 0;
    int last_algo = 0;            // LP_SIMPLEX_ALGO_* of the last run (which stamp buffer is current)
    int pivot_rule = LP_PIVOT_DANTZIG;   // lp_simplex_set_pivot_rule: read by every run
};

// simplex_driver.hip: the host side of a solve (upload, dispatch, the batch-and-poll loop, the stats record)
int check_canonical(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                    const int* basis, int n_orig);
// Is basis (m positions) the unit-vector basis of the column-major A, and are its costs all zero?  (*zero_costs is
// only meaningful when *identity holds.)  at_upper (per column, may be null): the columns flagged in it count negated.
void lp_slack_identity(const double* A, int m, const double* c, const int* basis, bool* identity, bool* zero_costs,
                       const int* at_upper = nullptr);
// Dynamic LDS above the default 48 KiB needs an opt-in.  The limit is an attribute of the kernel, not of a
// problem, so every run sets it for the size it is about to launch with.
hipError_t lp_lds_opt_in(const void* kernel, size_t bytes);
// lp_simplex_upload in its two halves.  alloc: the problem record of an m x n tableau with every device buffer, the
// pinned state block and the events; nothing is uploaded (c, n values or null: the costs lp_simplex_download
// evaluates).  install: from the column-major A, then b, then c staged in p->dT0 the tableau, the basis and computeBFS
// (identity / zero_costs: lp_slack_identity's verdict on what is staged); sets p->init_status and leaves the
// post-crash snapshot in p->dT0.  lp_mip_bounded_solve_large stages every rebuilt node on the device and installs it.
int lp_simplex_alloc(lp_context* ctx, int m, int n, const double* c, int maximize, int n_orig,
                     lp_simplex_problem** problem_out);
int lp_simplex_install(lp_simplex_problem* p, const int* basis_in, bool identity, bool zero_costs);
// simplex_driver.hip: what lp_simplex_two_phase_ex shares with lp_simplex_bounded_large (simplex_bounded_driver.hip).
using ProblemOwner = std::unique_ptr<lp_simplex_problem, void (*)(lp_simplex_problem*)>;   // frees on every return
// The phase-I problem of [A | b]: rows with b_i < -eps negated, then an identity of artificials, which is the basis N.
void auxiliary_problem(const double* A, int m, int n, const double* b, double eps, double* A1, double* b1, double* c1,
                       int* N);
// Phase I's verdict on its vertex xa: LP_INFEASIBLE under prefix's name when the artificials sum to more than eps.
int phase1_verdict(lp_context* ctx, const std::string& prefix, const double* xa, int m, int n, double eps);
// Pivots the artificials still in the phase-I basis N out (*pivots counts them); LP_SINGULAR when one cannot leave.
int drive_out_artificials(lp_simplex_problem* p, const std::string& prefix, const int* N, int m, int n, double eps,
                          int* pivots);
// The basis of p alone, after a run that ended with a positive status.
int download_basis(lp_simplex_problem* p, int* N);

// Each path's launch surface.  begin() queues the state-init launches of a run and returns how many it queued;
// queue(batch) queues `batch` pivots and returns the launches queued (a negative value is a HIP error).

// simplex_launch.hip: one select + one rank-1-update launch per pivot (the selector of p->pivot_rule)
int lp_launch_prepare(lp_simplex_problem* p);   // the selector's LDS: checked, opted in
int lp_launch_begin(lp_simplex_problem* p, double eps, int max_iter);
int lp_launch_queue(lp_simplex_problem* p, int batch);
void lp_simplex_launch_update(lp_simplex_problem* p);
// The crash of p's basis: m selector + update pairs, the verdict, the rows into position order; one host sync.  A
// tableau with rows behind the cost row (a second cost row) passes `wide`, the same problem seen with those rows
// counted in dev.m, and `staged`, which queues what fills their eta entries behind each step's selector: the step's
// update then runs on `wide` and carries them with the pivot's own arithmetic.  They stay where they are afterwards.
int lp_simplex_crash(lp_simplex_problem* p, lp_simplex_problem* wide = nullptr,
                     const std::function<void()>& staged = {});
int lp_simplex_price_out_identity(lp_simplex_problem* p);  // unit-vector basis with non-zero costs
int lp_simplex_force(lp_simplex_problem* p, int row, int col);  // host-chosen pivot on the current tableau
int lp_simplex_driveout(lp_simplex_problem* p, const int* positions, int count, int n_limit, double eps, int* applied);
int lp_simplex_phase2_costs(lp_simplex_problem* p, const double* cost, int n_real, int maximize, int n_orig);
int lp_simplex_extract_x(lp_simplex_problem* p, double* dx);

// simplex_launch.hip: the re-solve from a given basis (lp_simplex_resolve_run).  classify: *flags = bit 0 primal
// infeasible, bit 1 dual infeasible (one host sync); the dual path then queues the dual selector + rank-1 update.
int lp_simplex_classify(lp_simplex_problem* p, double eps, int* flags);
int lp_dual_prepare(lp_simplex_problem* p);
int lp_dual_queue(lp_simplex_problem* p, int batch);
// simplex_driver.hip: the batch-and-poll loop of the launch paths for pivot pairs queued outside it (queue(batch)
// queues `batch` pivots and returns the launches queued); returns once the state word has left kRunning.
int lp_poll_pivots(lp_simplex_problem* p, const std::function<int(int)>& queue);

// simplex_bounded_launch.hip: the bounded-variable selector + the rank-1 update per iteration (the entries and their
// host side are simplex_bounded_driver.hip's).  The bound state lives beside the tableau, one entry per tableau column.
struct BoundedLargeDev {
    double* U;    // dev.n: hi - lo, +inf for the artificials
    int* up;      // dev.n: 1 = the column is held complemented
    int* flips;   // bound flips since the start of the solve
    double* q;    // dev.ld: the quotients of the dual selector's ratio test
    double* w;    // dev.n: the Devex weights (LP_PIVOT_DEVEX), 1.0 when a primal loop starts; under LP_DUAL_DEVEX the
                  // first dev.m of them are the dual loop's, one per basis position, 1.0 when it starts
};
// rule: LP_PIVOT_DANTZIG (k_simplex_select_bounded), LP_PIVOT_BLAND or LP_PIVOT_DEVEX, checked by the caller; dual:
// the bounded dual selector in that selector's place (no pivot rule reaches it; lp_bounded_dual_prepare first), under
// dual_rule: LP_DUAL_DANTZIG (k_simplex_select_dual_bounded) or LP_DUAL_DEVEX, and dual_ratio: LP_DUAL_RATIO_TEXTBOOK
// (those two selectors) or LP_DUAL_RATIO_LONG_STEP (their bound-flipping forms), both checked by the caller
int lp_bounded_large_prepare(lp_simplex_problem* p, int rule);   // that selector's LDS: checked, opted in
int lp_bounded_large_queue(lp_simplex_problem* p, const BoundedLargeDev& bd, int batch, int rule, bool dual,
                           int dual_rule = LP_DUAL_DANTZIG, int dual_ratio = LP_DUAL_RATIO_TEXTBOOK);
// queued, all 1.0: the dev.n weights of a primal loop, or (dual) the dev.m of a dual loop
void lp_bounded_large_reset_weights(lp_simplex_problem* p, const BoundedLargeDev& bd, bool dual = false);
// The re-solve (lp_simplex_bounded_resolve_large).  classify: *flags = bit 0 some basis position outside its bounds,
// bit 1 dual infeasible (one host sync); the dual path then queues the bounded dual selector + rank-1 update.
int lp_bounded_large_classify(lp_simplex_problem* p, const BoundedLargeDev& bd, double eps, int* flags);
int lp_bounded_dual_prepare(lp_simplex_problem* p, int dual_rule = LP_DUAL_DANTZIG, int dual_ratio = LP_DUAL_RATIO_TEXTBOOK);

// mip_bounded_large.hip: the device side of lp_mip_bounded_solve_large's search (tests/ref/mip_bounded_ref.c steps 2
// to 5).  What a solved node was, written by the node kernel into pinned host memory:
enum { LP_MIPL_PRUNED = 0, LP_MIPL_INTEGRAL = 1, LP_MIPL_ABANDONED = 2, LP_MIPL_BRANCHED = 3, LP_MIPL_NOT_BASIC = 4 };
struct MipLargeResult {
    int what;          // LP_MIPL_*
    int j;             // the branching column (BRANCHED, NOT_BASIC)
    int un_negative;   // BRANCHED with the dive applied: the first child's new width U' is < 0
    int t;             // BRANCHED with the dive applied: the basis position of j, else -1
    double z;          // the node's objective
    double v;          // x_j of the branching column
    double xb_before, U_before, lo_before;   // BRANCHED with the dive applied: xB_t, U_j and lo_j as the bound change
                                             // found them (what a snapshot of the node holds in their place)
};
struct MipLargeDev {
    const double* A;        // m x n column-major, b (m), c (n): uploaded once per call
    const double* b;
    const double* c;
    const int* integer;     // n: the mask
    double* lo;             // n: the node's lower bounds (a dive up moves one)
    double* x;              // n: the node's vertex in the caller's variables
    double* xinc;           // n_orig: the incumbent
    int* rec_basis;         // max_depth x m: the basis recorded when a level branched
    int* rec_up;            // max_depth x n: and the flags
    MipLargeResult* result; // pinned host memory
    int n_orig, max_depth;
    double int_tol, gap;
};
// Stages [A' | b' | c'] of the node (lo = md.lo, U = bd.U, flags = bd.up) in p->dT0 for lp_simplex_install; queued.
void lp_mip_large_stage(lp_simplex_problem* p, const BoundedLargeDev& bd, const MipLargeDev& md);
// The node kernel on the LP_OPTIMAL tableau of a node at level L; found / zstar: the incumbent so far; dive: apply
// the first child's bound change when the node branches.  Queued; md.result is valid after the next stream sync.
void lp_mip_large_node(lp_simplex_problem* p, const BoundedLargeDev& bd, const MipLargeDev& md, int L, int found,
                       double zstar, int dive);
// Snapshots (lp_mip_bounded_solve_large_ex; tests/ref/mip_bounded_snapshots_ref.c steps 4' and 6').  A slot holds the
// (m+1) x ld tableau, then U and the node's lo (n doubles each, padded to 16 bytes): slot_bytes of device memory,
// 16-byte aligned.  The basis and the flags of its level are the record's (rec_basis, rec_up).
size_t lp_mip_large_slot_bytes(int m, int n);
// Queued: the live state into `slot` with the three values of r (the node kernel's LP_MIPL_BRANCHED result, dive
// applied) in place of the live ones, so the slot holds the node as it stood before the dive's bound change.
void lp_mip_large_save(lp_simplex_problem* p, const BoundedLargeDev& bd, const MipLargeDev& md, char* slot,
                       const MipLargeResult& r);
// Queued: `slot` and the record of `level` back into the live state, then step 5 for column j of value v to the side
// `down`.  md.result is valid after the next stream sync: LP_MIPL_BRANCHED with un_negative, or LP_MIPL_NOT_BASIC.
void lp_mip_large_second_child(lp_simplex_problem* p, const BoundedLargeDev& bd, const MipLargeDev& md, char* slot,
                               int level, int j, double v, int down);

// simplex_lookahead.hip: J pivots per select + rank-J-update launch pair
int lp_lookahead_pick_j(int m, int n);          // the shape test: 0 = the selector does not fit LDS
int lp_lookahead_prepare(lp_simplex_problem* p);
int lp_lookahead_begin(lp_simplex_problem* p, double eps, int max_iter);
// (with profiling on, the update launches are bracketed by upd_events while *timed < upd_events.size() / 2)
int lp_lookahead_queue(lp_simplex_problem* p, int batch, int* timed);
void lp_lookahead_launch_select(lp_simplex_problem* p);
void lp_lookahead_launch_update(lp_simplex_problem* p);

// simplex_overlap.hip: one launch per pivot, the update of pivot k beside the selection of pivot k+1
struct OverlapPlan {
    size_t shm;       // the selector's dynamic LDS (every workgroup of the launch is given it)
    int fast;         // the selector with the priced cost row in LDS
    int linear;       // the update as persistent linear shares (else a tile per workgroup)
    int nbx;          // column tiles of the update
    unsigned grid;    // workgroups per launch, the selector's included
    int k;            // launches of the pivot kernel queued so far in this run
};
bool lp_overlap_fits(int m);
bool lp_overlap_auto(int m);    // what LP_SIMPLEX_ALGO_AUTO requires of the shape
int lp_overlap_prepare(lp_simplex_problem* p);   // allocates the second tableau buffer (first use)
int lp_overlap_plan(lp_simplex_problem* p, OverlapPlan* plan);   // launch shape + the LDS opt-in
int lp_overlap_begin(lp_simplex_problem* p, double eps, int max_iter);
int lp_overlap_queue(lp_simplex_problem* p, OverlapPlan& plan, int batch);
int lp_overlap_finish(lp_simplex_problem* p);    // the final tableau back to dev.T after an odd pivot count

// simplex_resident.hip: the whole solve in one launch
int lp_resident_plan(int m, int n, ResidentDev* out);   // fills G/stride/mpad/offsets; 0 if the shape does not fit
// state init, hand-off areas cleared, then the kernel between res_ev0 and res_ev1
int lp_resident_launch(lp_simplex_problem* p, double eps, int max_iter);
// After the state word is back: *rerun = a hand-off timed out (last_error says where), nothing was written back and
// the solve is to be re-run on another path; LP_BAD_ARG instead under LP_RESIDENT_STRICT.
int lp_resident_finish(lp_simplex_problem* p, bool* rerun);
int lp_simplex_debug_division(lp_context* ctx, const double* num, const double* den, int n, double* fast_out, double* plain_out);

// basis_ranging.hip: alpha (m x n, row-major) = B^-1 A from a tableau [B | I | b] that lp_simplex_crash left in
// position order, one fma chain per entry in row order; queued on ctx's stream.
void lp_binv_times_a_launch(lp_context* ctx, const SimplexDev& s, const double* dA, int n, double* alpha);
