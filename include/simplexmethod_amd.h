/*
 * simplexmethod_amd.h — C ABI of the MI355X-native dense-LP hot path.
 *
 * The reference (haskell-md2/SimplexMethod) has no FFI/plugin interface: its
 * boundary is the C++ class API `Solver(const Canonical&)` + `solve()`
 * (/root/reference/src/SimplexSolover.h:285-328) and, by README intent
 * (README.md:27,40-42), the same shape for `EnumerationSolver`
 * (src/EnumerationSolver.h:3-10, an empty stub).  The functions below are what a
 * maintainer binds instead of the Eigen arithmetic inside those two classes; the
 * C++ wrappers in simplexmethod_amd/host/ (Solver, EnumerationSolver) are that
 * binding and keep the reference's names, arguments and exception behaviour.
 * See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - plain pointers and sizes only; caller allocates every output; no
 *     ownership transfer; no exceptions cross the ABI.
 *   - matrices are COLUMN-MAJOR fp64 (Eigen's default order, so the reference's
 *     `A.data()` can be passed as is); indices are 32-bit int; combination ranks
 *     are 64-bit unsigned.
 *   - m = rows of the canonical A, n = ALL canonical columns (slacks included),
 *     n_orig = Canonical::GetOriginalVariablesCount() (Canonical.cpp:151-154).
 *   - every entry point returns one of the LP_* codes below; negative values are
 *     HIP runtime failures (-(int)hipError_t); lp_last_error() has the text.
 *   - there is NO CPU fallback: without a usable gfx950 device
 *     lp_context_create fails and every other call needs a context.
 */
#ifndef SIMPLEXMETHOD_AMD_H
#define SIMPLEXMETHOD_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LP_ABI_VERSION 4 /* 2: lp_simplex_stats grew algo_used / fell_back; lp_enum_shard_abstain, lp_batched_shard_bounds; 3: LP_SIMPLEX_ALGO_OVERLAP, lp_enum_exact_division, lp_debug_reciprocal; 4: lp_debug_division; added within 4 (new entry points only): lp_simplex_two_phase_batched, lp_batched_two_phase_upload, lp_batched_phase_iters, lp_batched_path; LP_PIVOT_DANTZIG / LP_PIVOT_BLAND, lp_simplex_set_pivot_rule, lp_batched_set_pivot_rule, lp_simplex_solve_ex, lp_simplex_two_phase_ex, lp_simplex_solve_batched_ex, lp_simplex_two_phase_batched_ex; lp_simplex_resolve_run, lp_simplex_resolve, lp_simplex_resolve_batched, lp_batched_resolve_upload, lp_batched_set_start, lp_batched_resolve_iters; lp_basis_duals, lp_basis_duals_batched, lp_batched_duals, lp_basis_duals_fits; lp_basis_ranging, lp_basis_ranging_batched, lp_batched_ranging, lp_basis_ranging_fits; LP_CERT_NONE / LP_CERT_FARKAS / LP_CERT_RAY, lp_basis_certificate, lp_basis_certificate_batched, lp_batched_certificates, lp_basis_certificate_fits; lp_basis_parametric, lp_basis_parametric_batched, lp_batched_parametric, lp_basis_parametric_fits; lp_basis_parametric_cost, lp_basis_parametric_cost_batched, lp_batched_parametric_cost, lp_basis_parametric_cost_fits; lp_mip_solve, lp_mip_solve_batched, lp_batched_mip, lp_mip_fits; lp_simplex_bounded, lp_simplex_bounded_batched, lp_simplex_bounded_fits; LP_PIVOT_DEVEX, lp_batched_devex_fits; lp_basis_bounded_duals, lp_basis_bounded_duals_batched, lp_basis_bounded_ranging, lp_basis_bounded_ranging_batched, lp_basis_bounded_fits; lp_basis_bounded_parametric, lp_basis_bounded_parametric_batched, lp_basis_bounded_parametric_cost, lp_basis_bounded_parametric_cost_batched, lp_basis_bounded_parametric_fits, lp_basis_bounded_parametric_cost_fits; lp_simplex_bounded_ex, lp_simplex_bounded_batched_ex, lp_simplex_bounded_resolve_ex, lp_simplex_bounded_resolve_batched_ex, lp_simplex_bounded_rule_fits */

/* Status codes; the C++ wrappers map them back to the
 * reference's exception types and messages.                                     */
enum {
    LP_OPTIMAL = 0,     /* Solver::solve returned                  SimplexSolover.h:432-440 */
    LP_UNBOUNDED = 1,   /* std::runtime_error, objective unbounded SimplexSolover.h:442-444 */
    LP_ITER_LIMIT = 2,  /* std::runtime_error, iteration limit     SimplexSolover.h:450     */
    LP_SINGULAR = 3,    /* std::runtime_error "Singular basis matrix"        :125-126       */
    LP_INFEASIBLE = 4,  /* enumeration found no feasible basis                              */
    LP_BAD_ARG = 5      /* std::invalid_argument from Canonical's ctor, Canonical.cpp:27-46;
                           "basis index out of range", SimplexSolover.h:101                 */
};

/* Enumeration verdict for one basis subset. */
enum { LP_SUBSET_FEASIBLE = 0, LP_SUBSET_INFEASIBLE = 1, LP_SUBSET_SINGULAR = 2 };

typedef struct lp_context lp_context; /* one HIP device + stream + scratch */

int lp_abi_version(void);
int lp_device_count(void);
/* Binds HIP device `device` (must be gfx950-class; fails loudly otherwise).
 * `stream` may be NULL (the library creates its own non-blocking stream) or an
 * existing hipStream_t owned by the caller.                                      */
int lp_context_create(int device, void* stream, lp_context** ctx_out);
void lp_context_destroy(lp_context* ctx);
const char* lp_last_error(const lp_context* ctx);
const char* lp_status_string(int status);
int lp_context_sync(lp_context* ctx);

/* =========================================================================
 * Simplex  —  replaces Solver::solveWithBasis / simplexIter / computeBFS
 *             (SimplexSolover.h:408-451, :135-209, :117-133)
 * ========================================================================= */

/* One-shot: upload, solve on the GPU, download.
 * basis_in : Canonical::GetBasisIndices() (m entries, by basis position).
 * eps      : Solver::EPS (1e-9, SimplexSolover.h:13).  Every solve entry of this header that takes eps
 *            (single, re-solve, two-phase, batched, bounded, MIP) requires eps >= 0 (+0.0, -0.0 and +inf
 *            included) and returns LP_BAD_ARG for eps < 0 or NaN.
 * max_iter : MAX_ITER (10000, SimplexSolover.h:426).
 * x_out    : n_orig doubles = solve()'s return value (:435-439).
 * basis_out: m ints, final basis BY POSITION (the reference's local N, :419).
 * obj_out  : c . x (Canonical::Evaluate, Canonical.cpp:86).
 * iters_out: pivots executed.   Any of basis_out/obj_out/iters_out may be NULL. */
int lp_simplex_solve(lp_context* ctx, const double* A, int m, int n, const double* b,
                     const double* c, const int* basis_in, int maximize, int n_orig, double eps,
                     int max_iter, double* x_out, int* basis_out, double* obj_out, int* iters_out);

/* Pivot rules.  DANTZIG (the default everywhere): first largest reduced cost, ratio ties toward the
 * lowest basis position (SimplexSolover.h:152-196); it can cycle on degenerate LPs.  BLAND: the
 * smallest eligible non-basic index with d_j > eps (max) / d_j < -eps (min) enters; among the rows
 * with u_i > eps whose ratio xB_i / u_i is within eps of the smallest, the one whose basic variable
 * has the smallest index leaves.  Bland's rule never cycles, and usually takes more pivots.  It runs
 * on LP_SIMPLEX_ALGO_LAUNCH (AUTO picks it) and on the LDS form of the batched kernels.
 * DEVEX: primal Devex pricing with Dantzig's ratio test.  One fp64 weight w_j per column, all exactly
 * 1.0 at the start of every run of the primal loop (each lp_simplex_run, each phase of the two-phase
 * flow; the drive-out pivots neither read nor update weights; no other reset).  A non-basic column
 * that may enter with d_j > eps (max) / d_j < -eps (min) is scored s_j = (d_j * d_j) / w_j; the
 * largest score enters, exact ties to the smallest index (no eps on scores; none eligible: optimal).
 * The leaving row is Dantzig's.  Then, from the old pivot row r, the old pivot element u_r and the
 * old w_e:  w_j = fmax(w_j, (t * t) * w_e) with t = T[r][j] / u_r for every non-basic j != e (the
 * artificial columns of phase II included), and w_v = fmax(w_e / (u_r * u_r), 1.0) for the leaving
 * variable v.  No fused multiply-add in any of it.  Devex is no anti-cycling rule.  It is expected to
 * help on badly scaled or large LPs, where it takes several times fewer pivots than Dantzig's rule;
 * it runs where Bland's rule runs (LP_SIMPLEX_ALGO_LAUNCH, which AUTO picks, and the LDS form of the
 * batched kernels), i.e. on forms that are slower per pivot than the ones Dantzig's AUTO chooses
 * (chip-resident, overlapped, register-resident batched): on small well-scaled LPs it loses.     */
enum { LP_PIVOT_DANTZIG = 0, LP_PIVOT_BLAND = 1, LP_PIVOT_DEVEX = 2 };

/* lp_simplex_solve with a pivot rule (any other value: LP_BAD_ARG).                             */
int lp_simplex_solve_ex(lp_context* ctx, const double* A, int m, int n, const double* b,
                        const double* c, const int* basis_in, int maximize, int n_orig, double eps,
                        int max_iter, double* x_out, int* basis_out, double* obj_out, int* iters_out,
                        int pivot_rule);

/* Device-resident form (used by bench.py so that timed regions start with the
 * tableau already in HBM).                                                       */
typedef struct lp_simplex_problem lp_simplex_problem;

enum {
    LP_SIMPLEX_ALGO_AUTO = 0,
    LP_SIMPLEX_ALGO_LAUNCH = 1,    /* one select + one rank-1-update launch per pivot   */
    LP_SIMPLEX_ALGO_LOOKAHEAD = 2, /* J pivots staged by a one-workgroup selector, then
                                      one rank-J update pass over the tableau            */
    LP_SIMPLEX_ALGO_RESIDENT = 3,  /* one launch per solve: the tableau stays in the registers of
                                      co-resident workgroups, one per CU (32 columns each for
                                      m <= 512, 16 columns each for 512 < m <= 960; at most 256
                                      workgroups, i.e. n <= 8192 resp. n <= 4096), one all-to-all
                                      hand-off per pivot; AUTO's choice when the shape fits.  A
                                      hand-off that times out (the workgroups never became
                                      co-resident) re-runs the solve on another algorithm:
                                      lp_simplex_stats::fell_back                          */
    LP_SIMPLEX_ALGO_OVERLAP = 4    /* one launch per pivot: the rank-1 update of pivot k streams the
                                      tableau out of place while one more workgroup of the same launch
                                      selects pivot k+1 from the old tableau and pivot k's eta; shapes
                                      beyond the chip-resident ones (a second tableau buffer is
                                      allocated on first use)                                */
};

typedef struct lp_simplex_stats {
    int status;
    int pivots;             /* pivots executed                                            */
    int launches;           /* kernel launches issued                                      */
    float solve_ms;         /* HIP-event time of the whole solve on the library's stream  */
    float update_ms;        /* HIP-event time spent in tableau-update launches: the rank-1 / rank-J
                               update launches when lp_simplex_profile is on; for the chip-
                               resident algorithm the one kernel that runs every pivot (always) */
    int update_launches;    /* launches counted in update_ms                               */
    double bytes_per_pivot; /* algorithmic bytes of one rank-1 update: 16*m*(n+1)          */
    int algo_used;          /* LP_SIMPLEX_ALGO_* that produced the answer (never AUTO)             */
    int fell_back;          /* 1: the chip-resident algorithm was asked for (or chosen by AUTO), a
                               hand-off timed out and the solve was re-run on algo_used; the answer is
                               the same, the solve took >= 200 ms longer.  0 otherwise.              */
} lp_simplex_stats;

int lp_simplex_upload(lp_context* ctx, const double* A, int m, int n, const double* b,
                      const double* c, const int* basis_in, int maximize, int n_orig,
                      lp_simplex_problem** problem_out);
/* Restores the initial tableau (device-to-device) so a solve can be repeated.   */
int lp_simplex_reset(lp_simplex_problem* p);
int lp_simplex_run(lp_simplex_problem* p, double eps, int max_iter, int algo,
                   lp_simplex_stats* stats_out);
/* The pivot rule of the problem's next runs (LP_PIVOT_DANTZIG after upload).  Under LP_PIVOT_BLAND and
 * LP_PIVOT_DEVEX, AUTO runs LP_SIMPLEX_ALGO_LAUNCH and an explicit RESIDENT, LOOKAHEAD or OVERLAP is
 * LP_BAD_ARG.  The Devex weights (n doubles on the device) are allocated by the first Devex run.   */
int lp_simplex_set_pivot_rule(lp_simplex_problem* p, int pivot_rule);
/* on != 0: the next runs bracket every tableau-update launch with HIP events so that
 * lp_simplex_stats::update_ms / update_launches are filled (costs ~1-2 us per launch; off by
 * default, in which case those two fields are 0).                                         */
int lp_simplex_profile(lp_simplex_problem* p, int on);
/* trace_*: first trace_cap pivots (entering column, leaving POSITION); tableau_out:
 * (m+1) x (n+1) row-major, rows by basis position, row m = reduced costs,
 * column n = xB.  Every pointer may be NULL.                                      */
int lp_simplex_download(lp_simplex_problem* p, double* x_out, int* basis_out, double* obj_out,
                        int* trace_enter, int* trace_leave, int trace_cap, double* tableau_out);
void lp_simplex_free(lp_simplex_problem* p);

/* ---- Two-phase simplex ---------------------------------------
 * For canonical problems without a usable starting basis (Symmetrical min problems,
 * negative b).  Replaces the flow the reference sketches in code its public API cannot reach
 * (SimplexSolover.h:61-68 make_b_nonneg, :70-95 createAuxiliaryProblem, :331-381
 * replaceArtificialColumns, :383-406 twoPhaseSimplex), made consistent: rows with b < -eps
 * change sign; phase I minimises the sum of m artificials [A' | I] from their identity basis;
 * LP_INFEASIBLE iff that sum > eps; an artificial still basic leaves for the first non-basic
 * original column with |T[pos][cand]| > eps (none: LP_SINGULAR, dependent constraints); phase II
 * CONTINUES ON THE PHASE-I TABLEAU: the reduced-cost row is re-priced from the original costs
 * over the current basis, the artificial columns stay but are barred from entering (no second
 * upload, no re-inversion; the vertex carries phase I's rounding, ~1e-16 relative).  Every pivot
 * runs on the GPU.
 * iters_out (optional): 3 ints = pivots of phase I, drive-out pivots, pivots of phase II.       */
int lp_simplex_two_phase(lp_context* ctx, const double* A, int m, int n, const double* b,
                         const double* c, int maximize, int n_orig, double eps, int max_iter,
                         double* x_out, int* basis_out, double* obj_out, int* iters_out);
/* lp_simplex_two_phase with a pivot rule for phase I and phase II (the drive-out is the same).  */
int lp_simplex_two_phase_ex(lp_context* ctx, const double* A, int m, int n, const double* b,
                            const double* c, int maximize, int n_orig, double eps, int max_iter,
                            double* x_out, int* basis_out, double* obj_out, int* iters_out,
                            int pivot_rule);
/* ---- Re-solve from a given basis ---------------------------------------------------------------
 * For the loop solve, change b (tighten a row, branch) or c, solve again from the old optimal basis.
 * The basis is installed as lp_simplex_upload installs it (the crash; LP_SINGULAR if singular), then:
 *   - primal feasible (no xB_t < -eps): the plain primal simplex, exactly lp_simplex_run(AUTO);
 *   - else dual feasible (no non-basic d_j > eps for max, d_j < -eps for min): the dual simplex.  The
 *     leaving position is the EPS-hysteresis chain (min) over the xB_t < -eps in position order (none:
 *     LP_OPTIMAL); the entering column the same chain over d_j / T[r][j] (max) or -d_j / T[r][j] (min) of
 *     the non-basic j with T[r][j] < -eps, in index order (none: LP_INFEASIBLE).  max_iter bounds its pivots;
 *   - else LP_BAD_ARG: the basis is no valid start.
 * Dantzig's rule only: a problem or batch set to LP_PIVOT_BLAND or LP_PIVOT_DEVEX returns LP_BAD_ARG.
 * iters_out: 2 ints per LP = dual pivots, primal pivots (one of them is 0; the crash is not counted).
 * Note: lp_simplex_solve from a basis that is not primal feasible is NOT a valid re-solve.          */
/* On an lp_simplex_upload handle (after upload or lp_simplex_reset).  The dual simplex runs the launch
 * pair per pivot (stats_out->algo_used = LP_SIMPLEX_ALGO_LAUNCH).                                   */
int lp_simplex_resolve_run(lp_simplex_problem* p, double eps, int max_iter, int* iters_out,
                           lp_simplex_stats* stats_out);
/* One-shot: upload, re-solve, download (arguments as lp_simplex_solve; x and obj for LP_OPTIMAL only). */
int lp_simplex_resolve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                       const int* basis_in, int maximize, int n_orig, double eps, int max_iter, double* x_out,
                       int* basis_out, double* obj_out, int* iters_out);

/* Row `row` (0..m-1 by basis position, m = reduced costs) of the current tableau: n+1 doubles. */
int lp_simplex_row(lp_simplex_problem* p, int row, double* out);
/* One Gauss-Jordan pivot at (row, col) of the current tableau, chosen by the caller
 * (replaceArtificialColumns, :357-366: N(pos) = cand; Binv = F * Binv).                        */
int lp_simplex_force_pivot(lp_simplex_problem* p, int row, int col);

/* Times `iters` launches of the rank-1 update kernel alone on the problem's
 * current tableau (pivot element (row, col) must be non-zero; the tableau is
 * restored afterwards).  ms_per_launch = HIP-event time / iters.                  */
int lp_bench_rank1_update(lp_simplex_problem* p, int row, int col, int iters,
                          float* ms_per_launch_out);

/* The same for the look-ahead path's rank-J update: the selector stages one batch of J pivots
 * on the problem's initial tableau (call after lp_simplex_reset), then the update launch is
 * replayed `iters` times between two HIP events.  *pivots_per_launch_out = J actually staged;
 * algorithmic bytes per launch = J * 16*m*(n+1).  State is restored afterwards.            */
int lp_bench_rankj_update(lp_simplex_problem* p, int iters, float* ms_per_launch_out,
                          int* pivots_per_launch_out);

/* Diagnostic (not part of the drop-in surface): first call with cap_pivots > 0 turns the
 * selectors' per-phase cycle stamps on; a later call copies the stamps (s_memtime ticks) of the
 * last run into `out`: after a look-ahead run 8 per pivot for the first cap_pivots pivots; after a
 * chip-resident run 16 per-phase cycle sums over the solve for each of the first cap_pivots (<= 256)
 * workgroups.                                                                              */
int lp_debug_simplex_stamps(lp_simplex_problem* p, int cap_pivots, unsigned long long* out);

/* Batched simplex (BASELINE.json configs[4]): `batch` independent LPs of one
 * shape, one LP per workgroup.  Arrays are concatenated per LP: A batch*m*n
 * (each column-major), b batch*m, c batch*n, basis_in batch*m; outputs x_out
 * batch*n_orig, basis_out batch*m, obj_out/iters_out/status_out batch.  eps as lp_simplex_solve
 * (LP_BAD_ARG for eps < 0 or NaN, here and in lp_batched_run).               */
int lp_simplex_solve_batched(lp_context* ctx, int batch, const double* A, int m, int n,
                             const double* b, const double* c, const int* basis_in, int maximize,
                             int n_orig, double eps, int max_iter, double* x_out, int* basis_out,
                             double* obj_out, int* iters_out, int* status_out);
/* The same with a pivot rule.  Under LP_PIVOT_BLAND the batch runs the kernel's LDS form (every
 * shape that stays on the GPU fits it); the per-LP fallback passes the rule on.  Under LP_PIVOT_DEVEX
 * the LDS form carries n - m more doubles, the weights: a batch that runs one LP per workgroup and
 * whose carve no longer fits 160 KiB with them (lp_batched_devex_fits(m, n, 0) == 0) returns
 * LP_BAD_ARG from the run.                                                                       */
int lp_simplex_solve_batched_ex(lp_context* ctx, int batch, const double* A, int m, int n,
                                const double* b, const double* c, const int* basis_in, int maximize,
                                int n_orig, double eps, int max_iter, double* x_out, int* basis_out,
                                double* obj_out, int* iters_out, int* status_out, int pivot_rule);

typedef struct lp_batched_problem lp_batched_problem;
int lp_batched_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                      const double* c, const int* basis_in, int maximize, int n_orig,
                      lp_batched_problem** problem_out);
int lp_batched_run(lp_batched_problem* p, double eps, int max_iter, float* ms_out);
int lp_batched_download(lp_batched_problem* p, double* x_out, int* basis_out, double* obj_out,
                        int* iters_out, int* status_out);
void lp_batched_free(lp_batched_problem* p);
/* The pivot rule of the batch's next runs, plain or two-phase (LP_PIVOT_DANTZIG after upload).  */
int lp_batched_set_pivot_rule(lp_batched_problem* p, int pivot_rule);
/* 1 if the one-LP-per-workgroup kernel of a plain (two_phase == 0: (m+1) x (n-m+1) tableau, n - m weights)
 * or two-phase (two_phase != 0: (m+1) x (n+1) tableau, n weights) batch holds the shape under LP_PIVOT_DEVEX,
 * else 0.  A batch that runs one LP per workgroup under the other rules and has 0 here returns LP_BAD_ARG
 * from lp_batched_run under Devex; batches that go LP by LP anyway are not concerned.               */
int lp_batched_devex_fits(int m, int n, int two_phase);
/* The kernel form a plain m x n batch takes under LP_PIVOT_DANTZIG when it runs one LP per workgroup (host
 * arithmetic only: no context, no device).  out = {threads, rows_per_thread, aligned, dreg} of the
 * register-resident kernel: its workgroup size, its row array per updating thread, 1 if the columns are
 * assigned wave by wave with a wave of its own for xB, 1 if wave 0 keeps the reduced costs in registers; or
 * threads = 0 (all four zero) for the LDS tableau.  Returns 1 if the condensed tableau fits the
 * one-LP-per-workgroup path at all (n > m and (m+1) x (n-m+1) doubles within one CU's LDS), else 0 with out zeroed. */
int lp_batched_form(int m, int n, int out[4]);
/* BASELINE.json configs[4] "1 -> 8 GPUs": the LPs of a batch are independent, so participant `shard`
 * of `shards` (one process or host thread per GPU) uploads and solves the LPs [*lo, *hi) of the batch
 * and nobody exchanges anything (replicas of the code, no collective; the caller concatenates the
 * outputs).  The convention every binding uses: *lo = batch*shard/shards, *hi = batch*(shard+1)/shards
 * (64-bit arithmetic) - contiguous, disjoint, covering, sizes differing by at most one.             */
int lp_batched_shard_bounds(int batch, int shard, int shards, int* lo, int* hi);

/* Batched two-phase simplex: `batch` LPs of one shape WITHOUT a starting basis (Symmetrical MIN
 * problems, rows with b < 0, equality rows), one LP per workgroup; per LP exactly
 * lp_simplex_two_phase (same checks, same results).  Inputs as lp_simplex_solve_batched without
 * basis_in; x_out batch*n_orig, basis_out batch*m, obj_out batch, iters_out batch*3 (phase I,
 * drive-out, phase II), status_out batch.  x and obj are written for LP_OPTIMAL LPs only; the basis
 * always.  Shapes whose tableau ((m+1) x (n+1) doubles) does not fit one CU's LDS are solved by
 * lp_simplex_two_phase one LP after another.                                                     */
int lp_simplex_two_phase_batched(lp_context* ctx, int batch, const double* A, int m, int n,
                                 const double* b, const double* c, int maximize, int n_orig,
                                 double eps, int max_iter, double* x_out, int* basis_out,
                                 double* obj_out, int* iters_out, int* status_out);
/* The same with a pivot rule for phase I and phase II (LP_PIVOT_DEVEX: n more doubles of LDS, see
 * lp_batched_devex_fits(m, n, 1)).                                                               */
int lp_simplex_two_phase_batched_ex(lp_context* ctx, int batch, const double* A, int m, int n,
                                    const double* b, const double* c, int maximize, int n_orig,
                                    double eps, int max_iter, double* x_out, int* basis_out,
                                    double* obj_out, int* iters_out, int* status_out, int pivot_rule);
/* Device-resident form: a handle that lp_batched_run / _download / _free accept (run may be
 * repeated; lp_batched_download's iters_out is then the sum of the three counts per LP).          */
int lp_batched_two_phase_upload(lp_context* ctx, int batch, const double* A, int m, int n,
                                const double* b, const double* c, int maximize, int n_orig,
                                lp_batched_problem** problem_out);
/* The three pivot counts per LP (batch*3) of the last run; LP_BAD_ARG on a plain batch.          */
int lp_batched_phase_iters(lp_batched_problem* p, int* iters_out);
/* 1: one LP per workgroup on the GPU, 0: per-LP fallback (any kind of batch).                    */
int lp_batched_path(const lp_batched_problem* p);

/* Batched re-solve: `batch` LPs of one shape, each from its given basis, one LP per workgroup; per LP
 * exactly lp_simplex_resolve.  Inputs as lp_simplex_solve_batched; iters_out batch*2 (dual, primal),
 * status_out batch (per-LP statuses, LP_BAD_ARG for a basis that is no valid start).  Shapes beyond the
 * batched two-phase kernel's (lp_simplex_two_phase_batched) are re-solved one LP after another.     */
int lp_simplex_resolve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                               const double* c, const int* basis_in, int maximize, int n_orig, double eps,
                               int max_iter, double* x_out, int* basis_out, double* obj_out, int* iters_out,
                               int* status_out);
/* Device-resident form: a handle that lp_batched_run (repeatable), _download (iters_out = the sum of the
 * two counts), _path and _free accept.                                                              */
int lp_batched_resolve_upload(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                              const double* c, const int* basis_in, int maximize, int n_orig,
                              lp_batched_problem** problem_out);
/* Replaces b (batch*m) and/or the starting bases (batch*m) of a re-solve batch; either may be NULL; A and c
 * stay.  The branch-and-bound loop: download basis_out, change b, set_start, run.  LP_BAD_ARG on a plain
 * or two-phase batch or for a basis index outside [0, n).                                             */
int lp_batched_set_start(lp_batched_problem* p, const double* b, const int* basis_in);
/* The two pivot counts per LP (batch*2: dual, primal) of the last run; LP_BAD_ARG on another kind.   */
int lp_batched_resolve_iters(lp_batched_problem* p, int* iters_out);

/* ---- Dual solution at a basis ------------------------------------------------------------------
 * Shadow prices y (m), reduced costs d (n) and the dual objective w for the LP (A, b, c) as given and a
 * basis of m column indices (by position); the optimisation sense does not matter: y_i = dz/db_i.
 *   1. T = [B^T | c_B] (m x (m+1)): row t is column basis[t] of A followed by c[basis[t]];
 *   2. lp_simplex_upload's crash on T with the identity basis 0..m-1 (column t pivots on the unused row of
 *      first-max |T[i][t]|; LP_SINGULAR when minp <= DBL_EPSILON*m*maxp, or for a repeated index);
 *      y[t] = the right-hand side of the row that column t pivoted on;
 *   3. d[j] = c[j] - sum_i A[i][j] y[i], one fused multiply-add chain per column in row order; basic columns
 *      exactly 0.0;  4. w = b^T y, one chain in row order.
 * At an optimal basis: max problems have d <= eps, min problems d >= -eps, and w = c^T x.  A basis index
 * outside [0, n) is LP_BAD_ARG.  y, d and w are NaN for an LP whose status is not LP_OPTIMAL.  The bits do not
 * depend on the path.  Every output pointer is required.                                              */
/* One LP; returns its status (LP_OPTIMAL, LP_SINGULAR, LP_BAD_ARG).                                   */
int lp_basis_duals(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                   const int* basis, double* y_out, double* d_out, double* w_out);
/* `batch` LPs of one shape (arrays concatenated per LP as in lp_simplex_solve_batched; y_out batch*m,
 * d_out batch*n, w_out batch), one LP per workgroup when lp_basis_duals_fits(m), else one LP after
 * another; per-LP statuses in status_out (an index out of range: LP_BAD_ARG for that LP).             */
int lp_basis_duals_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                           const double* c, const int* basis, double* y_out, double* d_out, double* w_out,
                           int* status_out);
/* The duals of every LP of a batch handle (plain, two-phase or re-solve) at its final basis after
 * lp_batched_run: a resident handle reads A, b, c and the bases where the run left them, any other handle
 * uploads the inputs it keeps once.  LPs whose run status is not LP_OPTIMAL keep it in status_out and get
 * NaN.  LP_BAD_ARG before the first run.                                                              */
int lp_batched_duals(lp_batched_problem* p, double* y_out, double* d_out, double* w_out, int* status_out);
/* 1: m fits the one-LP-per-workgroup kernel (its LDS <= 160 KB: m <= 140), 0 otherwise.               */
int lp_basis_duals_fits(int m);

/* ---- RHS and cost ranging at a basis -----------------------------------------------------------
 * How far each b_i and each c_j can move, one at a time, before the given basis (m column indices by position)
 * stops being primal (b) or dual (c) feasible, and the variable that leaves or enters at each end.  The ranges
 * describe the basis passed in: its optimality is not checked (as lp_basis_duals).  At a degenerate optimum a
 * range can be narrower than the interval over which the optimal value stays linear.  Everything in fp64:
 *   1. B^-1 and xB by lp_basis_duals's crash applied to [B | I | b] (B's column t = A's column basis[t]);
 *   2. d: exactly lp_basis_duals's reduced costs;  3. alpha[t][j] = (B^-1 A)[t][j] for non-basic j, one fused
 *      multiply-add chain per entry in row order;
 *   4. row i: r_t = -xB[t] / B^-1[t][i]; over t with B^-1[t][i] > eps the lower end b_i + max r_t, over t with
 *      B^-1[t][i] < -eps the upper end b_i + min r_t; the leaving column basis[t] at each end;
 *   5. non-basic column j: max problem [-inf, c_j - d_j], min problem [c_j - d_j, +inf] (the finite end enters j).
 *      Basic column basis[t]: rho_j = d_j / alpha[t][j] over non-basic j with |alpha| > eps; max problem:
 *      alpha > eps gives the lower end c + max rho, alpha < -eps the upper end c + min rho (a min problem swaps
 *      the sides); the entering column j at each end.
 * The first index wins a tie (its own value is reported, signed zeros included).  An empty side is -inf / +inf
 * with index -1.  Outputs come in interleaved pairs: [2k] lower end, [2k+1] upper end.  LP_SINGULAR when either
 * crash is singular; LP_BAD_ARG for a basis index outside [0, n) or eps < 0 / NaN.  Values are NaN and indices -1
 * for an LP whose status is not LP_OPTIMAL.  The bits do not depend on the path.  Every output pointer is required. */
/* One LP; returns its status (LP_OPTIMAL, LP_SINGULAR, LP_BAD_ARG).  rhs_out / rhs_var_out 2m, cost_out /
 * cost_var_out 2n.                                                                                     */
int lp_basis_ranging(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                     const int* basis, int maximize, double eps, double* rhs_out, int* rhs_var_out,
                     double* cost_out, int* cost_var_out);
/* `batch` LPs of one shape and sense (arrays concatenated per LP as in lp_basis_duals_batched; outputs batch*2m and
 * batch*2n), one LP per workgroup when lp_basis_ranging_fits(m, n), else one LP after another; per-LP statuses in
 * status_out.                                                                                          */
int lp_basis_ranging_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                             const double* c, const int* basis, int maximize, double eps, double* rhs_out,
                             int* rhs_var_out, double* cost_out, int* cost_var_out, int* status_out);
/* The ranges of every LP of a batch handle (plain, two-phase or re-solve) at its final basis after lp_batched_run,
 * for the LP as the caller gave it (rows a two-phase run sign-flipped never show) and the handle's sense.  LPs
 * whose run status is not LP_OPTIMAL keep it in status_out and get NaN.  LP_BAD_ARG before the first run.  */
int lp_batched_ranging(lp_batched_problem* p, double eps, double* rhs_out, int* rhs_var_out, double* cost_out,
                       int* cost_var_out, int* status_out);
/* 1: the shape fits the one-LP-per-workgroup kernel (its LDS <= 160 KB: m <= 132 for n = m, 128 x 256, and every
 * batched two-phase / re-solve shape with m <= 132), 0 otherwise.                                      */
int lp_basis_ranging_fits(int m, int n);

/* ---- Farkas and unbounded-ray certificates at a basis ------------------------------------------
 * Evidence for an LP_INFEASIBLE or LP_UNBOUNDED verdict, computed after the fact at the basis the solver stopped at
 * (every solver path stops before it pivots on the failing row or column).  A basis index n+i (0 <= i < m) is the
 * artificial of row i, column s_i e_i with s_i = -1 when b[i] < -eps and +1 otherwise (the two-phase row flip), so
 * a phase-I basis passes as it is.  Everything in fp64:
 *   1. B^-1 and xB by lp_basis_ranging's crash on [B | I | b]; alpha[t][j] = (B^-1 A)[t][j], one fused
 *      multiply-add chain per entry in row order;
 *   2. phase-I case (an artificial is basic): f = -(sum of the rows of B^-1 at the artificial positions, in
 *      position order).  FARKAS when the artificials' values xB, summed in artificial-index order, exceed eps and
 *      every original column has g_j = f^T A_j >= -eps (one chain in row order);
 *   3. dual-simplex case (no artificial, some xB[t] < -eps): the first position t with xB[t] < -eps and
 *      alpha[t][j] >= -eps for every non-basic j gives FARKAS with f = B^-1[t][:] and index t;
 *   4. ray case (otherwise): d_j = c_j - sum_t c[basis[t]] alpha[t][j], one chain in position order.  These bits
 *      are not lp_basis_duals's d.  The first non-basic j with d_j > eps (max) or d_j < -eps (min) and
 *      alpha[t][j] <= eps for every t gives RAY: r[j] = 1, r[basis[t]] = -alpha[t][j], +0.0 elsewhere; index j.
 * A FARKAS vector satisfies A^T f >= -eps and b^T f < 0; a RAY satisfies A r = 0 (to rounding), r >= -eps and
 * c^T r = d_j.  value: b^T f (one chain in row order) or d_j; index: t, j, or -1 (phase I, NONE).  farkas (m) is
 * NaN unless the kind is FARKAS, ray (n) NaN unless it is RAY, value NaN for NONE.  A certificate is emitted only
 * when it passes its own eps test: at the eps boundary the answer is NONE, never a wrong vector.  LP_SINGULAR when
 * the crash is singular or an index repeats; LP_BAD_ARG for an index outside [0, n+m) or eps < 0 / NaN.  The bits
 * do not depend on the path.  Every output pointer is required.                                          */
enum { LP_CERT_NONE = 0, LP_CERT_FARKAS = 1, LP_CERT_RAY = 2 };
/* One LP; returns its status (LP_OPTIMAL: the certificate was computed and kind_out says what was found;
 * LP_SINGULAR, LP_BAD_ARG).  farkas_out m, ray_out n, one kind / value / index.                              */
int lp_basis_certificate(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c,
                         const int* basis, int maximize, double eps, int* kind_out, double* farkas_out,
                         double* ray_out, double* value_out, int* index_out);
/* `batch` LPs of one shape and sense (arrays concatenated per LP as in lp_basis_ranging_batched; farkas_out
 * batch*m, ray_out batch*n, kind / value / index / status batch), one LP per workgroup when
 * lp_basis_certificate_fits(m, n), else one LP after another; per-LP statuses in status_out.             */
int lp_basis_certificate_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b,
                                 const double* c, const int* basis, int maximize, double eps, int* kind_out,
                                 double* farkas_out, double* ray_out, double* value_out, int* index_out,
                                 int* status_out);
/* The certificates of a batch handle (plain, two-phase or re-solve) after lp_batched_run, at each LP's final basis,
 * for the LP as the caller gave it (never the rows a two-phase run sign-flipped) and the handle's sense.  Only LPs
 * whose run ended LP_INFEASIBLE or LP_UNBOUNDED get one; every other LP gets NONE and NaN.  status_out holds the run
 * status, or LP_SINGULAR (LP_BAD_ARG) when the certificate's crash (basis) fails.  LP_BAD_ARG before the first
 * run.                                                                                                  */
int lp_batched_certificates(lp_batched_problem* p, double eps, int* kind_out, double* farkas_out, double* ray_out,
                            double* value_out, int* index_out, int* status_out);
/* 1: the shape fits the one-LP-per-workgroup kernel (its LDS <= 160 KB: 128 x 256, and every batched two-phase /
 * re-solve shape with m <= 132), 0 otherwise.                                                           */
int lp_basis_certificate_fits(int m, int n);

/* ---- Parametric right-hand side from an optimal basis -------------------------------------------
 * The optimal value z*(t) = opt { c^T x : A x = b + t d, x >= 0 } for t from 0 up to t_max, walked exactly from the
 * given optimal basis (m column indices by position) by one dual-simplex pivot per breakpoint.  z* is piecewise linear
 * in t: concave for a max problem, convex for a min problem.  Everything in fp64:
 *   1. T = [A | b | d ; c | 0 | 0]; the basis is installed by lp_simplex_resolve's crash (skipped for the slack
 *      identity with zero costs), which updates the d column like any other: beta = B^-1 b, delta = B^-1 d;
 *   2. the basis must be primal feasible (no beta_t < -eps) and dual feasible (no non-basic d_j > eps for max,
 *      d_j < -eps for min) at t = 0, else LP_BAD_ARG (re-solve first);
 *   3. segment k from t_k (t_0 = +0.0): over positions t ascending with delta_t < -eps, tau_t = -beta_t / delta_t;
 *      the breakpoint is the first strict minimum (a tie keeps the first position), t* = tau > t_k ? tau : t_k.
 *      No candidate, or t* >= t_max: the path ends at t_max (LP_OPTIMAL).  Else the entering variable is the
 *      re-solve's dual chain over the blocking row r (non-basic j with T[r][j] < -eps, q_j = d_j / T[r][j] for max,
 *      -d_j / T[r][j] for min, the EPS-hysteresis chain in index order).  None: the path ends at t* (LP_INFEASIBLE:
 *      infeasible for every t > t*).  max_breaks pivots done: the path ends at t* (LP_ITER_LIMIT).  Else the oracle's
 *      pivot over every column and the cost row, t_{k+1} = t*;
 *   4. obj[k] = sum_t c[basis[t]] * fma(t_k, delta_t, beta_t) and slope[k] = sum_t c[basis[t]] * delta_t, each one
 *      fused multiply-add chain in position order with segment k's basis; enter[k] / leave[k]: the variables of the
 *      pivot that ends segment k.  The last segment has enter -1 and leave the blocking row's variable
 *      (LP_INFEASIBLE, LP_ITER_LIMIT) or -1 (ended at t_max).  obj[nseg] is the chain at the final end with the last
 *      basis; at an end of +inf it is obj[nseg-1] when the last slope is 0, else +inf / -inf by the slope's sign.
 * Outputs: nseg (1 .. max_breaks+1), t[0..nseg], obj[0..nseg], slope / enter / leave [0..nseg-1] and the final basis
 * by position.  Entries past the path are NaN (values) and -1 (indices).  LP_SINGULAR (a singular or repeated basis)
 * and LP_BAD_ARG give nseg 0, NaN / -1 and the given basis back.  LP_BAD_ARG also for a NULL d or output, t_max < 0 /
 * NaN, eps < 0 / NaN, max_breaks < 0 or a basis index outside [0, n).  The bits do not depend on the path. */
/* One LP; returns its status (LP_OPTIMAL, LP_INFEASIBLE, LP_ITER_LIMIT, LP_SINGULAR, LP_BAD_ARG).  t_out / obj_out
 * max_breaks+2, slope_out / enter_out / leave_out max_breaks+1, basis_out m.                              */
int lp_basis_parametric(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const int* basis, int maximize, const double* d, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* basis_out);
/* `batch` LPs of one shape and sense (arrays concatenated per LP as in lp_basis_ranging_batched; d batch*m; per-LP
 * strides max_breaks+2 for t / obj, max_breaks+1 for slope / enter / leave, m for basis_out), one LP per workgroup
 * when lp_basis_parametric_fits(m, n), else one LP after another; per-LP statuses in status_out.            */
int lp_basis_parametric_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const int* basis, int maximize, const double* d, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* basis_out, int* status_out);
/* The paths of every LP of a batch handle (plain, two-phase or re-solve, fallback handles included) after
 * lp_batched_run, from each LP's final basis, for the LP as the caller gave it (rows a two-phase run sign-flipped never
 * show) and the handle's sense; d is batch*m, the outputs as lp_basis_parametric_batched.  LPs whose run status is not
 * LP_OPTIMAL keep it in status_out and get nseg 0.  The handle's pivot rule does not matter.  LP_BAD_ARG before the
 * first run.                                                                                               */
int lp_batched_parametric(lp_batched_problem* p, const double* d, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* basis_out, int* status_out);
/* 1: the shape fits the one-LP-per-workgroup kernel (its LDS <= 160 KB, e.g. the batched two-phase 64 x 192 class),
 * 0 otherwise.                                                                                              */
int lp_basis_parametric_fits(int m, int n);

/* ---- Parametric cost from an optimal basis ------------------------------------------------------
 * The optimal value z*(t) = opt { (c + t g)^T x : A x = b, x >= 0 } for t from 0 up to t_max, walked exactly from the
 * given optimal basis (m column indices by position) by one primal pivot per breakpoint.  z* is piecewise linear in t:
 * convex for a max problem, concave for a min problem.  A negative direction of t is -g.  Everything in fp64:
 *   1. T = [A | b ; c | 0 ; g | 0]; the basis is installed by lp_simplex_resolve's crash over all m+2 rows (skipped
 *      for the slack identity with c_B = 0 and g_B = 0): row m holds the reduced costs d of c, row m+1 the reduced
 *      costs delta of g;
 *   2. the basis must be primal feasible (no xB_t < -eps) and dual feasible (no non-basic d_j > eps for max,
 *      d_j < -eps for min) at t = 0, else LP_BAD_ARG (re-solve first);
 *   3. segment k from t_k (t_0 = +0.0): over non-basic j ascending with delta_j > eps (max) or delta_j < -eps (min),
 *      tau_j = -d_j / delta_j; the breakpoint is the first strict minimum (a tie keeps the first index),
 *      t* = tau > t_k ? tau : t_k.  No candidate, or t* >= t_max: the path ends at t_max (LP_OPTIMAL).  Else the
 *      chosen column e enters and the leaving position is the primal ratio test over column e (ratios xB_i / u_i
 *      for u_i > eps, the EPS-hysteresis chain in position order).  None: the path ends at t* (LP_UNBOUNDED:
 *      unbounded for every t > t*).  max_breaks pivots done: the path ends at t* (LP_ITER_LIMIT).  Else the oracle's
 *      pivot over every column and both cost rows, t_{k+1} = t*;
 *   4. obj[k] = sum_t (c + t_k g)[basis[t]] * xB_t, with the cost entry fma(t_k, g, c), and slope[k] =
 *      sum_t g[basis[t]] * xB_t, each one fused multiply-add chain in position order with segment k's basis;
 *      enter[k] / leave[k]: the variables of the pivot that ends segment k.  The last segment has leave -1 and enter
 *      the column that would enter (LP_UNBOUNDED, LP_ITER_LIMIT) or -1 (ended at t_max).  obj[nseg] is the chain at
 *      the final end with the last basis; at an end of +inf it is obj[nseg-1] when the last slope is 0, else +inf /
 *      -inf by the slope's sign.
 * Outputs: as lp_basis_parametric: nseg (1 .. max_breaks+1), t[0..nseg], obj[0..nseg], slope / enter / leave
 * [0..nseg-1] and the final basis by position.  Entries past the path are NaN (values) and -1 (indices).  LP_SINGULAR
 * (a singular or repeated basis) and LP_BAD_ARG give nseg 0, NaN / -1 and the given basis back.  LP_BAD_ARG also for
 * a NULL g or output, t_max < 0 / NaN, eps < 0 / NaN, max_breaks < 0 or a basis index outside [0, n).  The bits do
 * not depend on the path. */
/* One LP; returns its status (LP_OPTIMAL, LP_UNBOUNDED, LP_ITER_LIMIT, LP_SINGULAR, LP_BAD_ARG).  g n; t_out /
 * obj_out max_breaks+2, slope_out / enter_out / leave_out max_breaks+1, basis_out m.                      */
int lp_basis_parametric_cost(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const int* basis, int maximize, const double* g, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* basis_out);
/* `batch` LPs of one shape and sense (arrays concatenated per LP as in lp_basis_ranging_batched; g batch*n; per-LP
 * strides max_breaks+2 for t / obj, max_breaks+1 for slope / enter / leave, m for basis_out), one LP per workgroup
 * when lp_basis_parametric_cost_fits(m, n), else one LP after another; per-LP statuses in status_out.       */
int lp_basis_parametric_cost_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const int* basis, int maximize, const double* g, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* basis_out, int* status_out);
/* The cost paths of every LP of a batch handle (plain, two-phase or re-solve, fallback handles included) after
 * lp_batched_run, from each LP's final basis, for the LP as the caller gave it (rows a two-phase run sign-flipped never
 * show) and the handle's sense; g is batch*n, the outputs as lp_basis_parametric_cost_batched.  LPs whose run status is
 * not LP_OPTIMAL keep it in status_out and get nseg 0.  The handle's pivot rule does not matter.  LP_BAD_ARG before
 * the first run.                                                                                           */
int lp_batched_parametric_cost(lp_batched_problem* p, const double* g, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* basis_out, int* status_out);
/* 1: the shape fits the one-LP-per-workgroup kernel (its LDS <= 160 KB, e.g. the batched two-phase 64 x 192 class),
 * 0 otherwise.                                                                                              */
int lp_basis_parametric_cost_fits(int m, int n);

/* =========================================================================
 * Integer LPs: depth-first branch-and-bound, one problem per workgroup (the definition is
 * tests/ref/mip_ref.c).  The columns j with integer[j] = 1 (j < n_orig; one mask of n entries for the whole batch)
 * must be integral.  The root starts from `basis` as lp_simplex_resolve does (primal feasible -> primal simplex, else
 * dual feasible -> dual simplex, else LP_BAD_ARG; singular -> LP_SINGULAR) and is bit-identical to it.  x_j is
 * integral iff min(f, 1-f) <= int_tol, f = x_j - floor(x_j); the most fractional marked variable branches (ties to
 * the lowest index), the side nearer to its value first.  Each branch appends one row and one slack (variable
 * n + level): the first child to the parent's final tableau in tableau form (dual simplex), the second child by a
 * crash from A, the path's branch rows and the parent's basis.  A node is pruned unless its LP optimum beats the
 * incumbent by more than gap.  Dantzig's rule only.
 *   - max_depth (0..64) bounds the appended rows: a fractional node there is abandoned and the search goes on;
 *     max_nodes (>= 1) bounds the node LP solves (the root is 1) and max_iter each node's pivots: either stops the
 *     search.  Any of the three makes the status LP_ITER_LIMIT with the incumbent kept.  A node whose crash gives
 *     LP_SINGULAR or LP_BAD_ARG stops the search with that status (not expected on well-conditioned input).
 *   - status: LP_OPTIMAL (the incumbent is optimal), LP_INFEASIBLE (no integer point, or the root is infeasible),
 *     LP_UNBOUNDED (the root relaxation), LP_ITER_LIMIT, LP_SINGULAR / LP_BAD_ARG (eps < 0 or NaN among others).
 *   - found_out 0/1; x_out (n_orig) and obj_out the incumbent, NaN without one; bound_out the best LP objective
 *     over the incumbent and the nodes left open or abandoned (equal to obj_out on LP_OPTIMAL; +-inf when the root
 *     relaxation is unbounded or unfinished; NaN with neither); stats_out[4] = nodes solved, dual pivots, primal
 *     pivots, deepest level (crash pivots not counted).
 *   - only shapes with lp_mip_fits(m, n, max_depth) run: the others get LP_BAD_ARG.  There is no per-LP host path.
 * ========================================================================= */
int lp_mip_solve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const int* basis, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out);
/* A batch of problems of one shape and one mask: A batch*m*n, b batch*m, c batch*n, basis batch*m; outputs x_out
 * batch*n_orig, obj_out / bound_out / found_out / status_out batch, stats_out batch*4.                          */
int lp_mip_solve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const int* basis, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out, int* status_out);
/* From the final bases of a plain, two-phase or re-solve batch after lp_batched_run (LP_BAD_ARG before the first
 * run, and for a batch set to LP_PIVOT_BLAND or LP_PIVOT_DEVEX).  LPs whose run did not end LP_OPTIMAL keep their status.  Outputs as
 * lp_mip_solve_batched.                                                                                         */
int lp_batched_mip(lp_batched_problem* p, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out, int* status_out);
/* 1: the search's LDS carve (the (m+max_depth+1) x (n+max_depth+1) tableau and the per-level records) fits one
 * CU's 160 KB and max_depth is in [0, 64]; 0 otherwise.                                                      */
int lp_mip_fits(int m, int n, int max_depth);

/* =========================================================================
 * Bounded variables: the two-phase bounded-variable primal simplex, one LP per workgroup (the
 * definition is tests/ref/bounded_ref.c).  Problem: opt c.x, A x = b, lo <= x <= hi with lo[n] finite and hi[n]
 * finite or +inf (lo_j == hi_j: a fixed column).  The variables are shifted to x - lo in [0, hi - lo]; an upper
 * bound is kept out of the tableau: the ratio test also stops a basic variable at its upper bound, an entering
 * variable that reaches its own upper bound first FLIPS to it (no pivot), and a column at its upper bound is held
 * complemented.  The phases are lp_simplex_two_phase's (rows with b' < -eps change sign, phase I over m artificials,
 * LP_INFEASIBLE iff their sum > eps, the same drive-out with LP_SINGULAR, phase II on the phase-I tableau with the
 * artificials barred).  Dantzig's rule (another rule: lp_simplex_bounded_ex).  With lo = 0 and hi = +inf the result is lp_simplex_two_phase's.
 *   - LP_BAD_ARG for a NaN or infinite lo_j, a NaN hi_j, eps < 0 or NaN, a NULL pointer or a shape beyond lp_simplex_bounded_fits
 *     (there is no per-LP host path); an LP with some hi_j < lo_j is LP_INFEASIBLE without an iteration.
 *   - max_iter bounds each phase's iterations; an iteration is a pivot or a bound flip.
 *   - outputs: x_out (n_orig) and obj_out (sum_{j<n} c_j x_j) for LP_OPTIMAL only; basis_out (m) and at_upper_out
 *     (n, 0/1: 1 = the column is held complemented, i.e. at its upper bound when non-basic) always; iters_out[4] =
 *     phase-I pivots, drive-out pivots, phase-II pivots, bound flips.  Every output pointer is required.
 * ========================================================================= */
int lp_simplex_bounded(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out);
/* A batch of LPs of one shape: A batch*m*n, b batch*m, c / lo / hi batch*n; outputs x_out batch*n_orig, basis_out
 * batch*m, at_upper_out batch*n, obj_out / status_out batch, iters_out batch*4.  A bad lo or hi in any LP refuses
 * the whole call (LP_BAD_ARG); an LP with hi < lo is LP_INFEASIBLE and the others are solved.                      */
int lp_simplex_bounded_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out);
/* 1: the kernel's LDS carve (the (m+1) x (n+1) tableau, hi - lo and lo per column) fits one CU's 160 KB (64 x 192
 * does), 0 otherwise.  A host call: no context, no device.                                                      */
int lp_simplex_bounded_fits(int m, int n);

/* ---- Bounded variables: shapes beyond one workgroup's LDS ------------------------------------------------------
 * The LP of lp_simplex_bounded on the tableau in HBM (the definition is still
 * tests/ref/bounded_ref.c, and the results equal it bit for bit): the flow of lp_simplex_two_phase with one selector
 * and one rank-1 update launch per iteration.  The selector takes the bounded ratio test; a bound flip is done inside
 * it (two columns, O(m)) and streams no tableau, a pivot whose leaving variable leaves at its upper bound is staged
 * complemented.  Arguments, outputs, statuses and refusals are lp_simplex_bounded's with one difference: there is no
 * lp_simplex_bounded_fits limit (the limits are lp_simplex_two_phase's: device memory for the (m+1) x (n+m+1)
 * tableau, and m <= 9980 for the selector's LDS).  At a shape that also fits LDS the result is lp_simplex_bounded's.
 *   - LP_BAD_ARG for a NaN or infinite lo_j, a NaN hi_j, eps < 0 or NaN, or a NULL pointer; an LP with some
 *     hi_j < lo_j is LP_INFEASIBLE without an iteration (zero counters, basis n + t, no flag).
 *   - max_iter bounds the pivots plus flips of each phase; iters_out[4] = phase-I pivots, drive-out pivots, phase-II
 *     pivots, bound flips.
 *   - Dantzig's rule; Bland's rule and Devex pricing at these shapes are lp_simplex_bounded_large_ex (with the _ex
 *     block below; m <= 9968 under LP_PIVOT_DEVEX).  The dual solution and ranging at these shapes are
 *     lp_basis_bounded_duals_large and lp_basis_bounded_ranging_large below, and the evidence for an LP_INFEASIBLE or
 *     LP_UNBOUNDED verdict is lp_basis_bounded_certificate_large; the parametric paths along b + t d and c + t g are
 *     lp_basis_bounded_parametric_large and lp_basis_bounded_parametric_cost_large.  The re-solve
 *     from a basis at these shapes is lp_simplex_bounded_resolve_large below, and branch and bound over the bounds is
 *     lp_mip_bounded_solve_large (with the bounded MIP block).  lp_simplex_bounded itself is unchanged and still
 *     refuses larger shapes.                                                                                      */
int lp_simplex_bounded_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out);
/* The re-solve of lp_simplex_bounded_resolve (below) on the tableau in HBM (the definition is
 * tests/ref/bounded_resolve_ref.c, and the results equal it bit for bit): after lp_simplex_bounded_large, tightening a
 * bound, fixing a column or moving b or c costs the m crash pivots that install the basis on the (m+1) x (n+1) tableau
 * (no artificial columns) plus the dual or primal pivots from there, instead of the whole two-phase solve.  The primal
 * loop is lp_simplex_bounded_large's phase II; the dual loop is one bounded dual selector and one rank-1 update launch
 * per pivot.  Arguments, outputs, statuses, refusals and iters_out[3] (dual pivots, primal pivots, bound flips) are
 * lp_simplex_bounded_resolve's with one difference: there is no lp_simplex_bounded_fits limit (the limits are device
 * memory for the tableau, and m <= 9960 for the selectors' LDS).  At a shape that also fits LDS every output equals
 * lp_simplex_bounded_resolve's.  Dantzig's rule (Bland's and Devex in the primal loop:
 * lp_simplex_bounded_resolve_large_ex, with the _ex block below), one LP per call; lp_simplex_bounded_resolve itself
 * is unchanged and still refuses larger shapes.  Every pointer is required.                                        */
int lp_simplex_bounded_resolve_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out);

/* ---- Bounded variables: the re-solve from a basis -------------------------------------------------------------
 * The LP of lp_simplex_bounded re-solved from basis_in (m, by position, every index in [0, n)) and at_upper_in (n,
 * 0/1), normally the basis_out and at_upper_out of an earlier solve, after a change of lo, hi, b or c (DESIGN.md
 * §4.5k; the definition is tests/ref/bounded_resolve_ref.c).  Under any change of lo, hi or b an optimal basis stays
 * dual feasible, so tightening a bound costs a few dual pivots instead of a two-phase solve.  The tableau is built on
 * the shifted variables with every flagged column held complemented, the basis is installed by lp_simplex_resolve's
 * crash (LP_SINGULAR: the given basis and flags are returned), and then:
 *   - no basic variable below its lower or above its finite upper bound by more than eps: the bounded primal loop of
 *     lp_simplex_bounded's phase II (pivots and bound flips; max_iter bounds their sum);
 *   - else, no reduced cost of the wrong sign beyond eps: the bounded dual simplex.  The leaving position is the most
 *     violated one (a variable above its upper bound is complemented first and leaves at that bound), the entering
 *     column lp_simplex_resolve's dual ratio test; no entering column: LP_INFEASIBLE.  max_iter bounds the dual pivots;
 *   - else LP_BAD_ARG: the basis is no valid start (in a batch: that LP's status, the others are solved).
 * An LP with some hi_j < lo_j is LP_INFEASIBLE with zero counters and the given basis and flags.  LP_BAD_ARG also for a
 * basis index outside [0, n), a flag that is not 0 or 1, a flag on a column with hi_j = +inf, and everything
 * lp_simplex_bounded refuses (in a batch these refuse the whole call).  Outputs as lp_simplex_bounded, except
 * iters_out[3] = dual pivots, primal pivots, bound flips (the crash is not counted).  With lo = 0, hi = +inf and no
 * flag the result is lp_simplex_resolve_batched's.  Shapes: lp_simplex_bounded_fits.                                */
int lp_simplex_bounded_resolve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out);
/* A batch of LPs of one shape: arrays as lp_simplex_bounded_batched, basis_in batch*m, at_upper_in batch*n, iters_out
 * batch*3.                                                                                                        */
int lp_simplex_bounded_resolve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out);

/* ---------------------------------------------------------------------------------------------------------------------
 * The bounded-variable simplex and its re-solve under a pivot rule.  Arguments and outputs are those of the entry
 * without _ex, with the rule appended: LP_PIVOT_DANTZIG runs the kernel of that entry and is bit-identical to it in
 * every output; any other value than the three rules is LP_BAD_ARG.  Only the iteration of the primal loop depends on
 * the rule (the definition is tests/ref/bounded_rules_ref.c); it holds in phase I and in phase II, and the drive-out is
 * the same under every rule.
 *   - LP_PIVOT_BLAND: the eligible column of smallest index enters.  The row values are Dantzig's bounded ratios,
 *     theta* = min(min_t v_t, U_e) exactly; among the rows with v_t <= theta* + eps, keyed by their basic variable, and
 *     the entering variable itself, keyed by its index, when U_e <= theta* + eps, the smallest key wins: a bound flip
 *     if it is the entering variable, else the pivot (after the complement when a_r < -eps).  The smallest-subscript
 *     rule for bounded variables: no cycling, e.g. on Beale's LP with boxed columns, where Dantzig's rule ends
 *     LP_ITER_LIMIT.
 *   - LP_PIVOT_DEVEX: one fp64 weight per column slot, 1.0 when each phase's loop (the re-solve's primal loop) starts;
 *     the eligible column of largest d*d/w enters, exact ties to the smallest index.  Ratio test, flip decision and
 *     complement are Dantzig's; a flip leaves the weights alone; before a pivot w_s = max(w_s, (T_rs/u_r)^2 w_e) and
 *     w_se = max(w_e/u_r^2, 1), as in lp_simplex_two_phase_batched_ex.
 * In the re-solve the rule governs the primal branch only: the crash, the classification and the dual branch are
 * unchanged, and their result under any rule is lp_simplex_bounded_resolve's bit for bit (the dual branch has a pricing
 * rule of its own: the _dual_ex entries and LP_DUAL_* below).  With lo = 0, hi = +inf and
 * no flag every output under a rule equals lp_simplex_two_phase_batched_ex's under that rule bit for bit.
 * Shapes: lp_simplex_bounded_rule_fits; a shape that fits plain but not with Devex's weights is LP_BAD_ARG under
 * LP_PIVOT_DEVEX, and nothing is launched.  The branch-and-bound over bounds stays with Dantzig's rule.            */
int lp_simplex_bounded_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule);
int lp_simplex_bounded_batched_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out, int pivot_rule);
int lp_simplex_bounded_resolve_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule);
int lp_simplex_bounded_resolve_batched_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out, int pivot_rule);
/* The same beyond one workgroup's LDS: lp_simplex_bounded_large and lp_simplex_bounded_resolve_large under a pivot
 * rule, one selector per rule on the tableau in HBM, each followed by the same rank-1 update launch.
 * LP_PIVOT_DANTZIG launches what the entry without _ex launches and equals it bit for bit; the entries without _ex
 * are these with LP_PIVOT_DANTZIG.  Any other value than the three rules is LP_BAD_ARG before anything else is looked
 * at, and no output is written.  The definitions are tests/ref/bounded_rules_ref.c and bounded_resolve_rules_ref.c, and
 * every output equals them bit for bit; at a shape where lp_simplex_bounded_rule_fits holds it also equals
 * lp_simplex_bounded_ex's / lp_simplex_bounded_resolve_ex's.  Devex keeps one weight per tableau column (the phase-I
 * artificials included) in device memory, all 1.0 when each primal loop starts.  There is no
 * lp_simplex_bounded_rule_fits limit; the limits are device memory for the tableau and the selector's LDS:
 * m <= 9980 under LP_PIVOT_DANTZIG and LP_PIVOT_BLAND, m <= 9968 under LP_PIVOT_DEVEX (its pricing keeps sixteen wave
 * results more), and m <= 9960 in the re-solve's dual branch under every rule.  Bland's rule is the one entry that
 * terminates on a cycling boxed LP at these shapes; it is slow everywhere else.                                       */
int lp_simplex_bounded_large_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule);
int lp_simplex_bounded_resolve_large_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule);
/* Host call, no context.  1: the shape runs under pivot_rule: lp_simplex_bounded_fits(m, n) for LP_PIVOT_DANTZIG and
 * LP_PIVOT_BLAND; under LP_PIVOT_DEVEX the LDS carve with n more doubles, the weights, must still fit 160 KiB.  0
 * otherwise, and for an unknown rule.                                                                                */
int lp_simplex_bounded_rule_fits(int m, int n, int pivot_rule);

/* The pricing rule of the bounded DUAL loop, the loop every warm re-solve from a dual feasible basis ends in (DESIGN.md
 * §4.5k3; the definition is tests/ref/bounded_resolve_dual_rules_ref.c, which every output equals bit for bit).  The
 * three entries take the arguments of their _ex entry with dual_rule appended.  pivot_rule governs the primal branch
 * only and dual_rule the dual branch only; a re-solve runs one of the two.
 *   - LP_DUAL_DANTZIG: the most violated position leaves (the EPS-hysteresis chain over v_t).  The entry launches
 *     exactly what its _ex entry launches and equals it bit for bit.
 *   - LP_DUAL_DEVEX: one fp64 reference weight per basis position, all exactly 1.0 when the dual loop starts.  With
 *     v_t the violation (xB_t below -eps, else U - xB_t below -eps for a finite U), the violated position of largest
 *     (v_t * v_t) / w_t leaves; exact ties go to the smallest position, a NaN score never wins, and there is no eps
 *     hysteresis.  The complement of a position violated above, the entering ratio test and the infeasible verdict
 *     are unchanged.  Before the pivot on (r, e), with a = T[r][e] after the complement: w_i = max(w_i, (T[i][e]/a)^2 w_r)
 *     for i != r, then w_r = max(w_r / a^2, 1).  Status and objective are those of LP_DUAL_DANTZIG up to rounding
 *     wherever that one ends optimal; the optimal basis and the pivot count may differ.
 * Any other dual_rule is LP_BAD_ARG before anything else is looked at, and no output is written.
 * Shapes: the two LDS entries need lp_simplex_bounded_dual_rule_fits (else LP_BAD_ARG, nothing launched).  The _large
 * entry keeps its m weights in device memory and has no such limit; its Devex dual selector keeps sixteen wave results
 * more in LDS than the plain one: m <= 9957 in the dual branch under LP_DUAL_DEVEX.
 * Not covered: the branch-and-bound entries (lp_mip_bounded_solve, _batched, _large and _large_ex, and their _ratio_ex
 * forms below) and the parametric paths keep Dantzig's dual rule, and the unbounded lp_simplex_resolve family is not
 * touched.  In the search the rule was measured on the host and left out: a node's dual loop is a handful of pivots,
 * too short for reference weights that restart at 1.0 to matter (32 435 dual pivots against 32 109 over 1800 nodes at
 * 32 x 96, under 2 % either way at every shape tried).                                              */
enum { LP_DUAL_DANTZIG = 0, LP_DUAL_DEVEX = 1 };
int lp_simplex_bounded_resolve_dual_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule, int dual_rule);
int lp_simplex_bounded_resolve_batched_dual_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out, int pivot_rule, int dual_rule);
int lp_simplex_bounded_resolve_large_dual_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule, int dual_rule);
/* Host call, no context.  A re-solve runs its primal or its dual loop, never both, so the two weight arrays share one
 * region: 1 when the LDS carve of lp_simplex_bounded_fits plus max(pivot_rule == LP_PIVOT_DEVEX ? n : 0,
 * dual_rule == LP_DUAL_DEVEX ? m : 0) doubles fits 160 KiB; 0 otherwise, and for an unknown rule of either kind.      */
int lp_simplex_bounded_dual_rule_fits(int m, int n, int pivot_rule, int dual_rule);

/* The ratio test of the bounded DUAL loop: how the entering column is chosen once a position r leaves (DESIGN.md
 * §4.5k4; the definition is tests/ref/bounded_resolve_long_step_ref.c, which every output equals bit for bit).  The
 * three entries take the arguments of their _dual_ex entry with dual_ratio appended.  dual_ratio governs the entering
 * step of the dual branch only: the checks, the crash, the classification, the primal branch, the leaving choice under
 * either dual rule and the complement of a position violated above are unchanged.
 *   - LP_DUAL_RATIO_TEXTBOOK: the column of smallest d_s / T[r][s] enters, whatever its own box.  The entry launches
 *     exactly what its _dual_ex entry launches and equals it in every output.
 *   - LP_DUAL_RATIO_LONG_STEP: the bound-flipping ratio test.  With e the candidate of that same chain: if U_e is
 *     finite and fma(-U_e, T[r][e], xB_r) < -eps, row r stays violated with e at its other bound, so e is flipped as
 *     the primal loop flips (xB_i = fma(-U_e, T[i][e], xB_i) for every row and the cost row, column e negated, its
 *     flag toggled) and the chain runs again on the same row; the first candidate whose flip would cure the violation
 *     is pivoted on.  A flip is O(m) where the pivot it replaces is O(m n).  No candidate left: LP_INFEASIBLE, with
 *     the basis and the flags as they stand, flips included.  Under LP_DUAL_DEVEX a flip leaves the weights alone.
 *     Status and objective are LP_DUAL_RATIO_TEXTBOOK's up to rounding wherever that one ends optimal; the optimal
 *     basis, the flags and the counts may differ.
 * max_iter bounds the dual pivots, as before; a dual iteration makes at most n flips.  iters_out[2] counts the dual
 * loop's flips as well as the primal loop's (a re-solve runs one of the two).
 * Any other dual_ratio is LP_BAD_ARG before anything else is looked at, and no output is written.
 * Shapes: the long-step kernels need no LDS beyond their textbook forms: lp_simplex_bounded_dual_rule_fits for the two
 * LDS entries, and the _large entry's limits on m are those of its _dual_ex entry.
 * The branch-and-bound over the bounds takes the same choice through lp_mip_bounded_solve_ratio_ex, _batched_ratio_ex
 * and _large_ratio_ex (below); its entries without that suffix keep the textbook test, and every one of them keeps
 * Dantzig's primal and dual pricing.  Not covered: the parametric paths keep the textbook ratio test, and the unbounded
 * lp_simplex_resolve family (no boxes, so nothing to flip) is not touched.                                          */
enum { LP_DUAL_RATIO_TEXTBOOK = 0, LP_DUAL_RATIO_LONG_STEP = 1 };
int lp_simplex_bounded_resolve_ratio_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule, int dual_rule, int dual_ratio);
int lp_simplex_bounded_resolve_batched_ratio_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int* status_out, int pivot_rule, int dual_rule, int dual_ratio);
int lp_simplex_bounded_resolve_large_ratio_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, double eps, int max_iter, double* x_out, int* basis_out, int* at_upper_out, double* obj_out, int* iters_out, int pivot_rule, int dual_rule, int dual_ratio);

/* ---- Bounded variables: branch-and-bound over the bounds ------------------------------------------------------
 * The LP of lp_simplex_bounded with the columns j < n_orig of integer[j] = 1 integral (one mask of n entries for the
 * whole batch), searched depth first from basis_in and at_upper_in, normally what lp_simplex_bounded returned
 * (the definition is tests/ref/mip_bounded_ref.c).  A branch changes one bound (hi_j = floor(v) or
 * lo_j = ceil(v)), so the tableau stays (m+1) x (n+1) at every depth, where lp_mip_solve appends a row and a slack per
 * level.  The root is lp_simplex_bounded_resolve's result bit for bit.  The integrality test, the branching variable
 * (most fractional, ties to the lowest index), the nearer side first and the pruning by gap are lp_mip_solve's.  The
 * first child changes the bound on the parent's final tableau (one held value moves) and runs the bounded dual
 * simplex; the second child is lp_simplex_bounded_resolve from the path's bounds and the basis and flags recorded when
 * the level branched.
 *   - LP_BAD_ARG for everything lp_simplex_bounded_resolve and lp_mip_solve refuse (max_depth in [0, 1024] here), and
 *     for a marked column whose lo_j, or whose finite hi_j, is not an integer (in a batch these refuse the whole call);
 *   - max_depth bounds the bound changes on a path (a fractional node there is abandoned), max_nodes (>= 1) the node
 *     LP solves (the root is 1), max_iter each node's pivots plus bound flips; status, found_out, x_out, obj_out and
 *     bound_out as lp_mip_solve.  A node LP that ends neither LP_OPTIMAL nor LP_INFEASIBLE stops the search with its
 *     status;
 *   - stats_out[5] = nodes solved, dual pivots, primal pivots, bound flips, deepest level (crash pivots not counted);
 *   - only shapes with lp_mip_bounded_fits(m, n, max_depth) run: the others get LP_BAD_ARG here, and are what
 *     lp_mip_bounded_solve_large below is for.                                                                     */
int lp_mip_bounded_solve(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out);
/* A batch of problems of one shape and one mask: arrays as lp_simplex_bounded_resolve_batched; outputs x_out
 * batch*n_orig, obj_out / bound_out / found_out / status_out batch, stats_out batch*5.  root_status (batch ints, may
 * be NULL) chains a cold lp_simplex_bounded_batched: an LP whose entry is not LP_OPTIMAL keeps that status, gets NaN /
 * 0 outputs and no search (its basis and flags are not read by the search, but must pass the checks: give zeros).  */
int lp_mip_bounded_solve_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, const int* root_status, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out, int* status_out);
/* 1: lp_simplex_bounded_fits' carve plus max_depth records of 24 + 4 m + 4 ceil(n / 32) bytes fits one CU's 160 KB and
 * max_depth is in [0, 1024] (64 x 192 at depth 64, 32 x 96 at 256, 16 x 40 at 1024); 0 otherwise.  A host call.      */
int lp_mip_bounded_fits(int m, int n, int max_depth);
/* The search of lp_mip_bounded_solve on the tableau in HBM (the definition is still
 * tests/ref/mip_bounded_ref.c, and every output equals it bit for bit), one problem per call.  The host drives the
 * depth-first search; A, b and c go up once, and the tableau, the bound state, the incumbent and the records' bases and
 * flags stay on the device.  A node that ended LP_OPTIMAL is evaluated by one launch (x, z, pruning, the branching
 * column, the record, the first child's bound change on the live tableau) and one host sync; the first child then runs
 * lp_simplex_bounded_resolve_large's dual loop where it stands, without a crash; a second child is staged on the device
 * from the persistent A and pays the m crash pivots that install the recorded basis.  Arguments, outputs, statuses,
 * refusals and stats_out[5] are lp_mip_bounded_solve's with one difference: there is no lp_mip_bounded_fits limit (the
 * limits are lp_simplex_bounded_resolve_large's, device memory for the tableau and m <= 9960 for the dual selector's
 * LDS, plus max_depth records of m + n ints in device memory; max_depth stays in [0, 1024]).  Refusals are checked
 * before anything is launched and leave the context usable.  At a shape that also fits LDS every output equals
 * lp_mip_bounded_solve's.  Dantzig's primal and dual rules at every node; lp_mip_bounded_solve itself is unchanged and
 * still refuses larger shapes.  Every pointer is required.
 *
 * lp_mip_bounded_solve_large_ex: the same search with up to `snapshots` = K tableau snapshots in device memory (DESIGN.md
 * §4.5l3; the definition is tests/ref/mip_bounded_snapshots_ref.c, and every output equals it bit for bit).  A node that
 * branches at level L and dives is saved as it stood before the dive's bound change (the tableau, U and the node's lo;
 * the basis and the flags are the level's record) in slot L mod K, which then belongs to level L; a second child whose
 * level still owns its slot is restored from it and continues exactly like a first child: the other side's bound change
 * on the restored tableau (one launch, one sync), then the bounded dual loop, with no staging, no crash and no
 * classification.  Any other second child is rebuilt as above.  With K >= max_depth every second child is restored; a
 * smaller ring keeps the K deepest pending levels, the ones depth-first search returns to first.
 *   - snapshots outside [0, 1024] is LP_BAD_ARG before anything else is looked at, and no output is written; every
 *     other refusal is lp_mip_bounded_solve_large's;
 *   - at most min(snapshots, max_depth) slots are allocated, each when the search first writes it (so a call takes at
 *     most lp_mip_bounded_snapshot_bytes(m, n, min(snapshots, max_depth)) for them); a failed allocation returns the
 *     negative HIP error, frees what the call took and leaves the context usable;
 *   - snapshots = 0 launches exactly what lp_mip_bounded_solve_large launches and equals it in every output;
 *     lp_mip_bounded_solve_large is this entry with 0 snapshots and a five-entry copy-out;
 *   - stats_out[7] = the five counters, then the second children restored, then the second children rebuilt;
 *   - with K > 0 the status, found_out and the nodes solved are those of K = 0 on every committed case and the objective
 *     agrees to rounding, but x_out may differ in its last bits: a restored child continues the parent's pivots where
 *     a rebuilt one crashes its basis afresh.  Dantzig's rules here too.                                             */
int lp_mip_bounded_solve_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out);
int lp_mip_bounded_solve_large_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out, int snapshots);
/* The three searches above with a choice of the ratio test of their dual loops (the definition is
 * tests/ref/mip_bounded_long_step_ref.c, which every output, the counters included, equals bit for bit).  Each takes
 * the arguments of lp_mip_bounded_solve, lp_mip_bounded_solve_batched or lp_mip_bounded_solve_large_ex (stats_out[7],
 * snapshots) with dual_ratio appended.
 *   - LP_DUAL_RATIO_TEXTBOOK launches exactly what the entry without the suffix launches and equals it in every
 *     output; those entries are these with LP_DUAL_RATIO_TEXTBOOK.
 *   - LP_DUAL_RATIO_LONG_STEP: every dual loop of the search, the install's at the root and at a rebuilt second child,
 *     a first child's on the live tableau and a restored second child's, enters by the bound-flipping ratio test of
 *     lp_simplex_bounded_resolve_ratio_ex under Dantzig's dual rule.  stats_out[3] counts the dual loops' flips as well
 *     as the primal loops'.  max_iter bounds a node's dual pivots alone in a dual loop (a dual iteration makes at most
 *     n flips) and its pivots plus flips in a primal loop, as before.  A node whose dual loop runs out of candidates,
 *     after flips or without one, is LP_INFEASIBLE and the search goes on.  A level's record, and its snapshot if any,
 *     are taken before the child's bound change, so a child's flips are in neither.  Node order, branching and pruning
 *     are unchanged; the nodes solved, the incumbent's last bits and the counters may differ from the textbook
 *     search's, and the objectives agree within gap plus rounding wherever both end LP_OPTIMAL.
 *   - Any other dual_ratio is LP_BAD_ARG before anything else is looked at, and no output is written.
 * Shapes: the long-step kernel needs no LDS beyond the textbook one, so lp_mip_bounded_fits is the limit of both LDS
 * entries; the _large entry's limits are lp_mip_bounded_solve_large_ex's.  Pricing stays Dantzig's, primal and dual
 * (see LP_DUAL_DEVEX above for the measured reason).                                                                */
int lp_mip_bounded_solve_ratio_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out, int dual_ratio);
int lp_mip_bounded_solve_batched_ratio_ex(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, const int* root_status, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out, int* status_out, int dual_ratio);
int lp_mip_bounded_solve_large_ratio_ex(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes, int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out, int snapshots, int dual_ratio);
/* Host call, no context.  *bytes_out = the device bytes `snapshots` slots take at m x n: snapshots x 8 x ((m + 1) ld +
 * 2 n2) with ld = n + 1 rounded up to a multiple of 8 and n2 = n rounded up to a multiple of 2 (the tableau's padded
 * rows, then U and the node's lo).
 * A caller sizes `snapshots` against free device memory with it.  LP_BAD_ARG (nothing written) for a NULL bytes_out,
 * m <= 0, n < m or snapshots outside [0, 1024].                                                                      */
int lp_mip_bounded_snapshot_bytes(int m, int n, int snapshots, unsigned long long* bytes_out);

/* ---- Bounded variables: the dual solution and ranging at a basis ------------------------------------------------
 * The LP of lp_simplex_bounded analysed at basis (m, by position, every index in [0, n)) and at_upper (n, 0/1),
 * normally the basis_out and at_upper_out of a solve (the definition is
 * tests/ref/bounded_sens_ref.c).  Everything is in the caller's original variables: a non-basic column is held at
 * v_j = hi_j when flagged, else lo_j; the flag of a basic column is not read.
 *   - b' = b - sum A_j v_j over the non-basic columns (one fma chain per row, j ascending, v_j != 0.0 only); xB and
 *     B^-1 by lp_basis_ranging's crash on [B | I | b']; x_out = xB on the basis and v elsewhere: the point the basis
 *     and the flags define;
 *   - y_out and d_out are lp_basis_duals' (basic d exactly 0.0); w_out = b.y + sum d_j v_j over the non-basic columns
 *     (lp_basis_duals' chain continued over j ascending, v_j != 0.0 only), which is c.x at an optimal basis.  Optimal
 *     means, under max, d_j <= eps at a lower bound and d_j >= -eps at an upper bound, under min the other way
 *     round; this is not checked;
 *   - RHS range of row i: with beta_t = B^-1[t][i], L_t / H_t the bounds of basis[t], the ratios (L_t - xB[t]) / beta_t
 *     and, H_t finite, (H_t - xB[t]) / beta_t (-xB[t] / beta_t when L_t == 0.0, as lp_basis_ranging); a ratio goes to
 *     the lower end (max) or the upper end (min) by the sign of beta_t beyond eps.  rhs_out[2i], [2i+1] = b_i + delta,
 *     rhs_var_out the leaving variable, rhs_side_out the bound it leaves at (0 lower, 1 upper); an empty side is
 *     -inf / +inf, -1 and -1.  The first position wins a tie;
 *   - cost ranges: the sense of a non-basic j is maximize XOR at_upper[j]: [-inf, c_j - d_j] if set, else
 *     [c_j - d_j, +inf] (a fixed column is ranged by its flag like any other); a basic column's ends are
 *     c + d_j / alpha[t][j] over the non-basic j with |alpha| > eps, a lower-end candidate (max) if (alpha > eps)
 *     equals j's sense, else an upper-end candidate (min).  cost_var_out is the entering column, -1 at an infinite
 *     end.  The first column wins a tie;
 *   - the status: LP_OPTIMAL, LP_SINGULAR (a crash failed; a repeated index ends here) or LP_INFEASIBLE (some
 *     hi_j < lo_j); then every value is NaN and every index and side -1.  LP_BAD_ARG for everything
 *     lp_simplex_bounded_resolve refuses about lo, hi, the basis and the flags, a NULL pointer (every output is
 *     required), for ranging eps < 0 or NaN, and a shape beyond lp_basis_bounded_fits (there is no per-LP host path).
 * With lo = 0, hi = +inf and no flag the results are lp_basis_duals' and lp_basis_ranging's bit for bit.            */
int lp_basis_bounded_duals(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, double* x_out, double* y_out, double* d_out, double* w_out);
/* A batch of LPs of one shape: arrays concatenated per LP (A batch*m*n, b batch*m, c / lo / hi / at_upper batch*n,
 * basis batch*m; x_out / d_out batch*n, y_out batch*m, w_out / status_out batch).  A bad bound, index or flag in any
 * LP refuses the whole call (LP_BAD_ARG); an LP with hi < lo is LP_INFEASIBLE and the others are computed.         */
int lp_basis_bounded_duals_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, double* x_out, double* y_out, double* d_out, double* w_out, int* status_out);
/* rhs_out / rhs_var_out / rhs_side_out 2m, cost_out / cost_var_out 2n: interleaved pairs (lower end, upper end).   */
int lp_basis_bounded_ranging(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, double eps, double* rhs_out, int* rhs_var_out, int* rhs_side_out, double* cost_out, int* cost_var_out);
/* A batch of LPs of one shape and sense: inputs as lp_basis_bounded_duals_batched; rhs_* batch*2m, cost_* batch*2n. */
int lp_basis_bounded_ranging_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, double eps, double* rhs_out, int* rhs_var_out, int* rhs_side_out, double* cost_out, int* cost_var_out, int* status_out);
/* 1: lp_simplex_bounded_fits(m, n) and the analysis kernel's LDS carve (lp_basis_ranging_fits' plus the held values
 * and the basic columns' bounds) fits one CU's 160 KB (64 x 192 does); 0 otherwise.  A host call.                   */
int lp_basis_bounded_fits(int m, int n);
/* The same two analyses beyond one workgroup's LDS, one LP per call (the definition is still
 * tests/ref/bounded_sens_ref.c, and every output equals it bit for bit, NaN and signed zeros included): what
 * lp_simplex_bounded_large returns can be analysed where it was solved.  The column codes, the held values and b' are
 * small kernels (b' one chain per row); lp_basis_ranging's single-LP path does the rest: the crash on [B | I | b']
 * ([B | b'] for the duals) by one selector and one rank-1 update launch per basis position on a tableau in HBM,
 * lp_basis_duals' path for y, d and b.y, B^-1 A as tiled chains, then one reduction kernel per range with the bounded
 * candidates.  Arguments, outputs, statuses and refusals are lp_basis_bounded_duals' and lp_basis_bounded_ranging's
 * with one difference: there is no lp_basis_bounded_fits limit.  The limit is device memory: two (m+1) x (2m+1)
 * tableaus ((m+1) x (m+1) for the duals) and, for ranging, the m x n matrix B^-1 A beside the inputs; the crash itself
 * takes any m.  At a shape where lp_basis_bounded_fits holds every output equals the entry's without _large.  With
 * lo = 0, hi = +inf and no flag the results are lp_basis_duals' and lp_basis_ranging's.  There is no batched form;
 * lp_basis_bounded_duals and lp_basis_bounded_ranging themselves are unchanged and still refuse larger shapes.       */
int lp_basis_bounded_duals_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, double* x_out, double* y_out, double* d_out, double* w_out);
int lp_basis_bounded_ranging_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, double eps, double* rhs_out, int* rhs_var_out, int* rhs_side_out, double* cost_out, int* cost_var_out);

/* ---- Bounded variables: Farkas and unbounded-ray certificates at a basis ----------------------------------------
 * Evidence for an LP_INFEASIBLE or LP_UNBOUNDED verdict of lp_simplex_bounded, lp_simplex_bounded_resolve or
 * lp_mip_bounded_solve, computed after the fact at the basis_out (m, by position, every index in [0, n+m): n+i is the
 * artificial of row i) and at_upper_out (n, 0/1) they stopped at (the definition is
 * tests/ref/bounded_certificate_ref.c).  Everything is fp64 and in the caller's original variables, as in
 * lp_basis_bounded_duals: a non-basic column is held at v_j = hi_j when flagged, else lo_j; the flag of a basic column
 * is not read.
 *   1. b' = b - sum A_j v_j is lp_basis_bounded_duals' chain; b0 = b - sum A_j lo_j (one fma chain per row, j ascending,
 *      lo_j != 0.0 only) decides the artificial of row i, the column s_i e_i with s_i = -1 when b0_i < -eps and +1
 *      otherwise: lp_simplex_bounded's row flip, so its phase-I basis passes as it is;
 *   2. B^-1 and xB by lp_basis_ranging's crash on [B | I | b']; alpha[t][j] = (B^-1 A)[t][j], one fma chain per entry
 *      in row order;
 *   3. a weight vector g over the original columns passes the sign test when every non-basic j has g_j >= -eps if held
 *      at lo_j and g_j <= eps if held at hi_j (basic columns are not tested; a fixed column is tested by its flag);
 *   4. phase-I case (an artificial is basic): f = -(sum of the rows of B^-1 at the artificial positions, in position
 *      order), g_j = f^T A_j.  FARKAS when the artificials' xB, summed in artificial-index order, exceed eps and g
 *      passes.  value = b'^T f (one chain in row order), index -1;
 *   5. dual-simplex case (no artificial, some position violated: xB[t] < L_t - eps, or xB[t] > H_t + eps with H_t
 *      finite; L_t, H_t the bounds of basis[t]): the first violated t whose row passes gives FARKAS with index t; below:
 *      f = B^-1[t][:], g = alpha[t][:]; above: f = -B^-1[t][:], g = -alpha[t][:].  value = b'^T f, then - L_t (when
 *      L_t != 0.0) below, + H_t above: xB[t] - L_t or H_t - xB[t] up to rounding;
 *   6. ray case (otherwise): d_j = c_j - sum_t c[basis[t]] alpha[t][j], one chain in position order (lp_basis_certificate's
 *      d, not the duals').  The first non-basic, unflagged j with hi_j = +inf, d_j > eps (max) or d_j < -eps (min), and
 *      for every t alpha[t][j] <= eps and (alpha[t][j] >= -eps or H_t = +inf) gives RAY: r[j] = 1,
 *      r[basis[t]] = -alpha[t][j], +0.0 elsewhere; value d_j, index j.
 * What a certificate proves, with g = A^T f.  FARKAS: f^T b < min over the box of f^T A x = sum_j min(g_j lo_j,
 * g_j hi_j), so no x in the box satisfies A x = b.  RAY: A r = 0 (to rounding), r >= -eps, r_k <= eps wherever hi_k is
 * finite, and c^T r = d_j of the improving sign.  A certificate is emitted only when it passes its own eps test: at the
 * eps boundary the answer is NONE, never a wrong vector.  Outputs as lp_basis_certificate (the LP_CERT_* kinds; farkas m,
 * NaN unless FARKAS; ray n, NaN unless RAY; value NaN for NONE; index), every pointer required.
 *   - the status: LP_OPTIMAL (computed; kind_out says what was found), LP_SINGULAR (the crash failed or an index
 *     repeats) or LP_INFEASIBLE (some hi_j < lo_j: crossed bounds need no vector); the last two with NONE, NaN and -1.
 *     LP_BAD_ARG for everything lp_basis_bounded_duals refuses about lo, hi and the flags, a basis index outside
 *     [0, n+m), eps < 0 or NaN, a NULL pointer and a shape beyond lp_basis_bounded_certificate_fits (there is no per-LP
 *     host path).
 * With lo = 0, hi = +inf and no flag every output is lp_basis_certificate's bit for bit.                          */
int lp_basis_bounded_certificate(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, double eps, int* kind_out, double* farkas_out, double* ray_out, double* value_out, int* index_out);
/* A batch of LPs of one shape and sense: arrays as lp_basis_bounded_duals_batched; farkas_out batch*m, ray_out batch*n,
 * kind / value / index / status batch.  run_status (batch ints, may be NULL) chains a bounded solve, re-solve or
 * branch-and-bound: an LP whose entry is neither LP_INFEASIBLE nor LP_UNBOUNDED keeps that status, gets NONE / NaN / -1
 * and its basis is not crashed (it must still pass the checks); an LP whose certificate was computed keeps its entry as
 * its status too (LP_OPTIMAL without run_status), as in lp_batched_certificates.  A bad bound, index or flag in any LP
 * refuses the whole call (LP_BAD_ARG); a singular basis and crossed bounds are that LP's status.                    */
int lp_basis_bounded_certificate_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, const int* run_status, int maximize, double eps, int* kind_out, double* farkas_out, double* ray_out, double* value_out, int* index_out, int* status_out);
/* 1: lp_simplex_bounded_fits(m, n) and the certificate kernel's LDS carve (lp_basis_certificate_fits' plus b', the held
 * values and the basic columns' bounds) fits one CU's 160 KB (64 x 192 does); 0 otherwise.  A host call.            */
int lp_basis_bounded_certificate_fits(int m, int n);
/* The same certificate beyond one workgroup's LDS, one LP per call (the definition is still
 * tests/ref/bounded_certificate_ref.c, steps 1-6 above, and every output equals it bit for bit, NaN and signed zeros
 * included): a verdict of lp_simplex_bounded_large or lp_simplex_bounded_resolve_large can be backed by evidence where
 * it was reached.  The column codes, the held values, b' and b0 are lp_basis_bounded_duals_large's small kernels (b0 is
 * the b' chain with lo held); lp_basis_certificate's single-LP path does the rest: the crash on [B | I | b'] with the
 * artificial columns s_i e_i explicit, by one selector and one rank-1 update launch per basis position on a tableau in
 * HBM, B^-1 A as tiled chains, then three kernels that choose the case and reduce under the box's rules (the first
 * position and the first column are decided by index, every chain is one thread's).  Arguments, outputs, statuses and
 * refusals are lp_basis_bounded_certificate's with one difference: there is no lp_basis_bounded_certificate_fits limit.
 * The limit is device memory: two (m+1) x (2m+1) tableaus and the m x n matrix B^-1 A beside the inputs.  At a shape
 * where lp_basis_bounded_certificate_fits holds every output equals lp_basis_bounded_certificate's; with lo = 0,
 * hi = +inf and no flag every output equals lp_basis_certificate's.  Crossed bounds are LP_INFEASIBLE before a repeated
 * index or a singular basis is LP_SINGULAR, as the definition orders them.  There is no batched form;
 * lp_basis_bounded_certificate, its _batched form and _fits are unchanged and still refuse larger shapes.            */
int lp_basis_bounded_certificate_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, double eps, int* kind_out, double* farkas_out, double* ray_out, double* value_out, int* index_out);

/* ---- Parametric right-hand side and parametric cost of a bounded-variable LP (the definition is
 * tests/ref/bounded_parametric_ref.c, numbered steps in its header) ----
 * lp_basis_parametric and lp_basis_parametric_cost for A x = b, lo <= x <= hi: every breakpoint of
 *   z*(t) = opt { c.x : A x = b + t d, lo <= x <= hi }        (lp_basis_bounded_parametric, d of m entries), or of
 *   z*(t) = opt { (c + t g).x : A x = b, lo <= x <= hi }      (lp_basis_bounded_parametric_cost, g of n entries)
 * for t from 0 up to t_max (+inf allowed), from the basis[m] and at_upper[n] that lp_simplex_bounded, its re-solve or
 * lp_mip_bounded returned at t = 0.  The bounds do not move with t.
 *   - the tableau is lp_simplex_bounded_resolve's (x = lo + x', flagged columns held complemented) with d as a second
 *     right-hand column or g as a second cost row; the given basis is installed by its crash and must be primal and
 *     dual feasible at t = 0 under eps (no position below 0 or above its width, no improving reduced cost), else
 *     LP_BAD_ARG: re-solve first;
 *   - RHS path: per segment the first strict minimum over the positions of tau = -beta_t / delta_t (delta_t < -eps) and
 *     tau = (U_t - beta_t) / delta_t (delta_t > eps, U_t finite); t* = max(tau, t_k).  The blocking variable leaves by
 *     one dual pivot (the re-solve's entering chain over its row, read complemented when it is blocked above).  Ends:
 *     LP_OPTIMAL at t_max, LP_INFEASIBLE at t* when nothing can enter (no feasible point beyond), LP_ITER_LIMIT at t*
 *     after max_breaks pivots.  For max z* is concave in t, for min convex;
 *   - cost path: per segment the first strict minimum over the non-basic columns in index order of tau = -d_j / delta_j
 *     (delta_j > eps for max, < -eps for min); the column enters by lp_simplex_bounded's ratio test: a pivot (the
 *     leaving variable may stop at its upper bound) or a bound flip, which is recorded as a breakpoint with
 *     enter = leave.  Ends: LP_OPTIMAL at t_max, LP_UNBOUNDED at t* (no row blocks and the column has no upper bound),
 *     LP_ITER_LIMIT at t* after max_breaks pivots and flips.  For max z* is convex in t, for min concave;
 *   - outputs as lp_basis_parametric (nseg_out; t_out / obj_out max_breaks+2; slope_out / enter_out / leave_out
 *     max_breaks+1; basis_out m; NaN / -1 past the path), obj and slope in the caller's variables (a non-basic column
 *     counts at the bound it is held at), and beside them side_out (max_breaks+1): the bound at which leave_out[k]
 *     stops, 0 lower, 1 upper, -1 where leave_out[k] is -1 (for a flip: the bound flipped to), and at_upper_out (n): the
 *     flags that go with basis_out.  Every pointer is required;
 *   - the status: the path's end as above; LP_SINGULAR (the crash failed or an index repeats), LP_INFEASIBLE with
 *     nseg 0 (some hi_j < lo_j) and LP_BAD_ARG for a start that is not optimal: these give nseg 0, NaN / -1 and the
 *     given basis and flags back.  LP_BAD_ARG also for everything lp_basis_bounded_duals refuses about lo, hi, the
 *     flags and the basis, t_max < 0 or NaN, eps < 0 or NaN, max_breaks < 0, a NULL pointer and a shape beyond the
 *     path's fits call (there is no per-LP host path; nothing is launched).
 * With lo = 0, hi = +inf and no flag every output shared with lp_basis_parametric / lp_basis_parametric_cost equals
 * theirs bit for bit, side_out is 0 wherever leave_out >= 0 and at_upper_out is 0.                                 */
int lp_basis_bounded_parametric(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, const double* d, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* side_out, int* basis_out, int* at_upper_out);
int lp_basis_bounded_parametric_cost(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, const double* g, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* side_out, int* basis_out, int* at_upper_out);
/* A batch of LPs of one shape and sense, one LP per workgroup: input arrays as lp_basis_bounded_duals_batched, d batch*m
 * or g batch*n; output arrays and per-LP strides as lp_basis_parametric_batched, side_out the size of leave_out,
 * at_upper_out batch*n, status_out batch.  run_status (batch ints, may be NULL) chains lp_simplex_bounded_batched or
 * lp_simplex_bounded_resolve_batched: an LP whose entry is not LP_OPTIMAL keeps it, gets nseg 0, NaN / -1 and its basis
 * and flags back, and is not crashed.  A bad bound, index or flag in any LP refuses the whole call (LP_BAD_ARG); a
 * singular basis, crossed bounds and a start that is not optimal are that LP's status.                              */
int lp_basis_bounded_parametric_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, const int* run_status, int maximize, const double* d, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* side_out, int* basis_out, int* at_upper_out, int* status_out);
int lp_basis_bounded_parametric_cost_batched(lp_context* ctx, int batch, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, const int* run_status, int maximize, const double* g, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* side_out, int* basis_out, int* at_upper_out, int* status_out);
/* 1: lp_simplex_bounded_fits(m, n) and the path's LDS carve (the bounded re-solve's with one more right-hand column,
 * or one more cost row, plus hi, c, g and the slot of every column) fits one CU's 160 KB (64 x 192 does for both); 0
 * otherwise.  Host calls, no context.                                                                              */
int lp_basis_bounded_parametric_fits(int m, int n);
int lp_basis_bounded_parametric_cost_fits(int m, int n);
/* The same two paths beyond one workgroup's LDS, one LP per call (the definition is still
 * tests/ref/bounded_parametric_ref.c, steps 1-5, R1-R3 and C1-C3, and every output equals it bit for bit on every
 * status, NaN fills, signed zeros, side_out and at_upper_out included): after lp_simplex_bounded_large or
 * lp_simplex_bounded_resolve_large the whole of z*(t) along b + t d or c + t g costs one crash and one selector +
 * rank-1 update launch pair per breakpoint on the tableau in HBM, instead of one re-solve (and its m crash pivots)
 * per guessed t.  The tableau is the bounded re-solve's (shifted variables, flagged columns complemented, b' its
 * chain).  RHS path: [A' | d | b'], d barred from entering, so the update carries both right-hand columns and a row
 * blocked above is staged complemented without touching the tableau.  Cost path: two cost rows and ONE crash, the g'
 * row carried through each crash step by the step's own update.  Per breakpoint the selector's last wave runs the
 * obj and slope chains while the other fifteen reduce tau, choose the entering column or the leaving row (or flip the
 * bound in place) and stage the pivot.  Arguments, outputs, statuses and refusals are lp_basis_bounded_parametric's
 * and lp_basis_bounded_parametric_cost's with one difference: there is no _fits limit.  The limits are device
 * memory (two tableaus of (m+1) x (n+2), or (m+2) and (m+1) rows of n+1) and the selectors' dynamic LDS, 24 m + 416
 * bytes (RHS) or 40 m + 448 bytes (cost) against 156 KiB: m <= 6638 and m <= 3982, else LP_BAD_ARG with a message
 * and nothing launched.  Crossed bounds are LP_INFEASIBLE (nseg 0) after every LP_BAD_ARG and before a repeated index
 * or a singular basis is LP_SINGULAR, as the definition orders them.  At a shape where the _fits call holds every
 * output equals the LDS entry's; with lo = 0, hi = +inf and no flag every output shared with lp_basis_parametric /
 * lp_basis_parametric_cost equals theirs, side_out is 0 wherever leave_out >= 0 and at_upper_out is 0.  There is no
 * batched form; the LDS entries, their _batched forms and the _fits calls are unchanged and still refuse larger
 * shapes.                                                                                                          */
int lp_basis_bounded_parametric_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, const double* d, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* side_out, int* basis_out, int* at_upper_out);
int lp_basis_bounded_parametric_cost_large(lp_context* ctx, const double* A, int m, int n, const double* b, const double* c, const double* lo, const double* hi, const int* basis, const int* at_upper, int maximize, const double* g, double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out, int* side_out, int* basis_out, int* at_upper_out);

/* =========================================================================
 * Enumeration — EnumerationSolver (src/EnumerationSolver.h:3-10 is a stub; spec
 * README.md:27,40-42; per-basis kernel = Canonical::GetBasicSolution /
 * IsFeasibleBasis / Evaluate, Canonical.cpp:165-197, :79-87).
 * Semantics: rank k in [0, C(n,m)) = k-th sorted
 * m-subset in lexicographic order; per subset a Gauss-Jordan solve with partial
 * pivoting; singular / infeasible (some xB < -1e-9) / feasible; winner = best
 * objective, ties within 1e-9 broken towards the smallest rank.
 * ========================================================================= */

uint64_t lp_binom(int n, int k); /* C(n,k), 0 on overflow */
/* Shard `shard` of `shards` contiguous rank ranges of EQUAL ESTIMATED COST for the shared-prefix
 * enumeration (the rank space shards across the GPUs of a node): cost(x) = x +
 * 160 * (depth m-7 tree nodes before subset x) — late prefixes have few subsets per node, and
 * equal-size shards differ by 1.5x in run time.  Pure host arithmetic; the solver's answer does
 * not depend on where the cuts are (tie rule).  Small problems get equal-size ranges.         */
int lp_enum_shard_bounds(int n, int m, int shard, int shards, uint64_t* begin_out,
                         uint64_t* end_out);

/* One-shot single-GPU solve.  counts_out[3] = {feasible, infeasible, singular}. */
int lp_enum_solve(lp_context* ctx, const double* A, int m, int n, const double* b,
                  const double* c, int maximize, int n_orig, double* x_out, int* basis_out,
                  uint64_t* rank_out, double* obj_out, uint64_t* counts_out);

typedef struct lp_enum_problem lp_enum_problem;

enum {
    LP_ENUM_ALGO_AUTO = 0,
    LP_ENUM_ALGO_DIRECT = 1, /* one independent m x m solve per subset                   */
    LP_ENUM_ALGO_PREFIX = 2  /* shared-prefix elimination over the combination tree
                                (bit-identical results, far fewer flops): 6 <= m <= 16 with
                                2 <= n-m <= 16 on the tuned kernels; 7 <= m <= 16 with any
                                n <= 64, or 17 <= m <= 32 with n-m <= 32, on the general one;
                                AUTO takes it for ranges of 2^15 subsets or more (2^8 for m > 16)         */
};

typedef struct lp_enum_stats {
    float kernel_ms;    /* HIP-event time of the enumeration kernel(s)                    */
    uint64_t subsets;   /* subsets processed                                              */
    int launches;
} lp_enum_stats;

int lp_enum_upload(lp_context* ctx, const double* A, int m, int n, const double* b,
                   const double* c, int maximize, lp_enum_problem** problem_out);
/* Pass 1 over the shard [rank_begin, rank_end): best objective over feasible
 * subsets (-inf/+inf if none) and the three counts.  This is what each GPU runs
 * on its slice of the rank space; the caller then reduces zbest over GPUs
 * (one RCCL all-reduce).                                                          */
int lp_enum_range(lp_enum_problem* p, uint64_t rank_begin, uint64_t rank_end, int algo,
                  double* zbest_out, uint64_t* counts_out, lp_enum_stats* stats_out);
/* Pass 2: smallest feasible rank in [rank_begin, rank_end) whose objective is
 * within tol of zstar on the better-or-equal side; UINT64_MAX if none.           */
int lp_enum_first_within(lp_enum_problem* p, uint64_t rank_begin, uint64_t rank_end, double zstar,
                         double tol, uint64_t* rank_out);
/* Vertex of one rank: x (n_orig), sorted basis (m), objective, verdict.          */
int lp_enum_vertex(lp_enum_problem* p, uint64_t rank, int n_orig, double* x_out, int* basis_out,
                   double* obj_out, int* verdict_out);
void lp_enum_free(lp_enum_problem* p);
/* 1 if the problem's leaf kernels divide plainly: a pass of the default kernels (fast reciprocal,
 * the same bits for a pivot magnitude within [2^-500, 2^500]) met a pivot outside that range on a
 * subset that was not singular anyway, and was repeated; later passes start there.  0 otherwise.  */
int lp_enum_exact_division(const lp_enum_problem* p);
/* Diagnostic (not part of the drop-in surface): the leaf kernels' fast reciprocal and the plain
 * division 1.0 / x[i], both computed on the device, for the parity test of the two.              */
int lp_debug_reciprocal(lp_context* ctx, const double* x, int n, double* fast_out, double* plain_out);
/* Diagnostic (not part of the drop-in surface): the chip-resident simplex's quotient by the pivot element (the
 * division's own instruction sequence without its range scaling, applied only to operands inside [2^-500, 2^501) or a
 * zero numerator) and the plain division num[i] / den[i], both computed on the device, for the parity test.      */
int lp_debug_division(lp_context* ctx, const double* num, const double* den, int n, double* fast_out, double* plain_out);

/* ---- Enumeration sharded over the GPUs of a node (README.md:27,40-42) ------
 * One participant per GPU — a process, or a host thread of one process — each with its own
 * lp_context and its own lp_enum_problem (the tiny problem is replicated).  Participant `rank`
 * of `world` enumerates shard lp_enum_shard_bounds(n, m, rank, world) with no data-path
 * collective; the only exchange is ONE all-gather of a 48-byte record per participant (best
 * score, smallest rank within 1e-9 of it, the three counts, status) — over RCCL/xGMI for
 * lp_comm_create_rccl communicators.  A second all-gather happens only when two shards hold
 * different vertices within 1e-9 of the optimum.  Results are identical on every participant and
 * for every world size (tie rule).                                                            */
typedef struct lp_comm lp_comm;
/* 128 bytes (ncclUniqueId): one participant calls this and hands the bytes to the others (file,
 * environment, MPI, a TCP store ...).  RCCL is loaded on first use (dlopen).                   */
int lp_comm_unique_id(void* id_out_128_bytes);
/* Collective: every participant calls it with the same id; blocks until all `world` have joined.
 * The communicator is bound to ctx's device and stream.                                        */
int lp_comm_create_rccl(lp_context* ctx, int rank, int world, const void* unique_id, lp_comm** comm_out);
/* `world` communicators for host threads of ONE process, exchanging through host memory;
 * participants may share a device (more shards than GPUs: what the one-GPU tests use).         */
int lp_comm_create_local(int world, lp_comm** comms_out /* world entries */);
int lp_comm_rank(const lp_comm* c);
int lp_comm_world(const lp_comm* c);
void lp_comm_destroy(lp_comm* c);
/* comm == NULL: a single participant (no exchange).  Outputs as lp_enum_solve (x_out and basis_out
 * may both be NULL: the winning rank, objective and counts then come straight from the exchange and
 * no vertex is evaluated); counts_out[3] are the node-wide totals.  Every participant must call it (a failing one still takes part in the
 * exchange, and every participant returns its status).                                          */
int lp_enum_solve_sharded(lp_comm* comm, lp_enum_problem* p, int n_orig, double* x_out, int* basis_out,
                          uint64_t* rank_out, double* obj_out, uint64_t* counts_out);
/* A participant that cannot enumerate (its context, upload or communicator set-up failed) calls this
 * INSTEAD of lp_enum_solve_sharded, so that the others are not left waiting in the exchange: it
 * contributes a failed record and returns `status` (LP_BAD_ARG if LP_OPTIMAL was passed); every other
 * participant's lp_enum_solve_sharded returns that status.  lp_enum_solve_sharded(comm, NULL, ...)
 * does the same with LP_BAD_ARG.                                                                 */
int lp_enum_shard_abstain(lp_comm* comm, int status);

#ifdef __cplusplus
}
#endif
#endif
