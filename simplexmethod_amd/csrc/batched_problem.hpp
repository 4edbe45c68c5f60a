// batched_problem.hpp — device-side description of a batch of same-shape LPs.
#pragma once

#include "lp_internal.hpp"

// The launch of every one-LP-per-workgroup kernel: d.batch workgroups of `threads`, `shm` bytes of dynamic LDS (the
// attribute first: the carves go beyond the default limit), on the context's stream.
template <class Dev>
int lp_launch_per_lp(lp_context* ctx, void (*kernel)(Dev), int threads, size_t shm, const Dev& d) {
    LP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)shm));
    hipLaunchKernelGGL(kernel, d.batch, threads, shm, ctx->stream, d);
    LP_HIP(ctx, hipGetLastError());
    return LP_OPTIMAL;
}

// The block-size rule of the kernels that hold a whole tableau of `cells` entries in LDS.  Small tableaus: four waves,
// so that several LPs share a CU; the rest: sixteen.
template <class Dev>
int lp_launch_per_lp(lp_context* ctx, size_t cells, void (*k256)(Dev), void (*k1024)(Dev), size_t shm, const Dev& d) {
    if (cells <= 4096) return lp_launch_per_lp(ctx, k256, 256, shm, d);
    return lp_launch_per_lp(ctx, k1024, 1024, shm, d);
}

struct BatchedDev {
    int batch, m, n;
    int pitch;        // row pitch (doubles) of the condensed LDS tableau, odd
    int maximize;
    int max_iter;
    double eps;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    const int* basis_in;    // batch x m
    double* x;              // batch x n  (full vertex)
    int* basis_out;         // batch x m  (by position)
    int* iters;             // batch
    int* status;            // batch
    unsigned long long* stamps;   // diagnostic (LP_BATCHED_STAMPS): 32 per-phase cycle sums of workgroup 0; nullptr = off
    int stamps_reg;               // LP_BATCHED_STAMPS=reg: the register form's instrumented instantiation (else the LDS form's)
    int pad_stamps;
};

// batched_simplex.hip
size_t lp_batched_lds_bytes(int m, int n, int* pitch_out);
int lp_batched_launch(lp_context* ctx, const BatchedDev& d, int pivot_rule);   // LP_PIVOT_BLAND, LP_PIVOT_DEVEX: the LDS form
size_t lp_batched_devex_lds_bytes(int m, int n);   // the LDS form's carve + n - m weights

// A batch of same-shape LPs solved by the two-phase flow, one LP per workgroup (batched_two_phase.hip).
struct BatchedTwoPhaseDev {
    int batch, m, n;        // n = canonical columns (the m artificials are implicit)
    int pitch;              // row pitch (doubles) of the LDS tableau, odd, >= n + 1
    int maximize;
    int max_iter;           // per phase
    double eps;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    double* x;              // batch x n  (full vertex)
    int* basis_out;         // batch x m  (by position)
    int* iters;             // batch x 3  (phase I, drive-out, phase II)
    int* status;            // batch
};

// batched_two_phase.hip
size_t lp_batched_two_phase_lds_bytes(int m, int n, int* pitch_out);
bool lp_batched_two_phase_fits(int m, int n);
size_t lp_batched_two_phase_devex_lds_bytes(int m, int n);   // the carve + n weights
int lp_batched_two_phase_launch(lp_context* ctx, const BatchedTwoPhaseDev& d, int pivot_rule);

// A batch of same-shape LPs re-solved from given bases, one LP per workgroup (batched_resolve.hip): the
// primal simplex when a basis is primal feasible, the dual simplex when it is only dual feasible.
struct BatchedResolveDev {
    int batch, m, n;
    int pitch;              // row pitch (doubles) of the LDS tableau: lp_batched_two_phase_lds_bytes
    int maximize;
    int max_iter;
    double eps;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    const int* basis_in;    // batch x m
    double* x;              // batch x n  (full vertex)
    int* basis_out;         // batch x m  (by position)
    int* iters;             // batch x 2  (dual pivots, primal pivots)
    int* status;            // batch
};

// batched_resolve.hip (the shapes of lp_batched_two_phase_fits)
int lp_batched_resolve_launch(lp_context* ctx, const BatchedResolveDev& d);

// The dual solution at given bases, one LP per workgroup (basis_duals.hip): y = B^-T c_B by the crash on
// [B^T | c_B], d = c - A^T y, w = b^T y.
struct BasisDualsDev {
    int batch, m, n;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    const int* basis;       // batch x m (by position)
    const int* run_status;  // batch, or nullptr: an LP whose entry is not LP_OPTIMAL keeps it and gets NaN
    double* y;              // batch x m
    double* d;              // batch x n
    double* w;              // batch
    int* status;            // batch
};

// basis_duals.hip
size_t lp_basis_duals_lds_bytes(int m);
int lp_basis_duals_launch(lp_context* ctx, const BasisDualsDev& d);   // lp_basis_duals_fits(m) shapes
// One LP of any m on the device (the basis in range): the crash by the single-LP launch pair, then the reduced
// costs; dA .. dbasis and dy, dd, dw are device pointers.  Returns LP_OPTIMAL / LP_SINGULAR (outputs untouched).
int lp_basis_duals_device(lp_context* ctx, const double* dA, int m, int n, const double* db, const double* dc,
                          const int* dbasis, double* dy, double* dd, double* dw);

// RHS and cost ranging at given bases, one LP per workgroup (basis_ranging.hip): B^-1 and xB by the crash on
// [B | I | b] (kept in place), d as basis_duals.hip, alpha = B^-1 A_N, then the ratio reductions.  Outputs in
// interleaved pairs (lower end, upper end).
struct BasisRangingDev {
    int batch, m, n;
    int maximize;
    double eps;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    const int* basis;       // batch x m (by position)
    const int* run_status;  // batch, or nullptr: an LP whose entry is not LP_OPTIMAL keeps it and gets NaN
    double* rhs;            // batch x 2m
    int* rhs_var;           // batch x 2m: the leaving column at each end
    double* cost;           // batch x 2n
    int* cost_var;          // batch x 2n: the entering column at each end
    int* status;            // batch
};

// basis_ranging.hip
size_t lp_basis_ranging_lds_bytes(int m, int n);
int lp_basis_ranging_launch(lp_context* ctx, const BasisRangingDev& d);   // lp_basis_ranging_fits(m, n) shapes
// One LP of any shape on the device (the basis in range, eps >= 0): the crash on [B | I | b] by the single-LP launch
// pair, d by lp_basis_duals_device, B^-1 A, then the reductions; every pointer is a device pointer.  Returns
// LP_OPTIMAL / LP_SINGULAR (outputs untouched).
int lp_basis_ranging_device(lp_context* ctx, const double* dA, int m, int n, const double* db, const double* dc,
                            const int* dbasis, int maximize, double eps, double* drhs, int* drhs_var, double* dcost,
                            int* dcost_var);

// Farkas and unbounded-ray certificates at given bases, one LP per workgroup (basis_certificate.hip): B^-1 and xB
// by the ranging crash on [B | I | b] (kept in place; basis index n+i is the artificial s_i e_i of row i), then the
// case's alpha chains and first-index reductions.
struct BasisCertificateDev {
    int batch, m, n;
    int maximize;
    double eps;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    const int* basis;       // batch x m (by position), indices in [0, n+m)
    const int* run_status;  // batch, or nullptr: only LPs whose entry is LP_INFEASIBLE / LP_UNBOUNDED get a
                            // certificate, the others keep their entry and get NONE
    int* kind;              // batch: LP_CERT_*
    double* farkas;         // batch x m
    double* ray;            // batch x n
    double* value;          // batch
    int* index;             // batch
    int* status;            // batch
};

// basis_certificate.hip
size_t lp_basis_certificate_lds_bytes(int m, int n);
int lp_basis_certificate_launch(lp_context* ctx, const BasisCertificateDev& d);   // lp_basis_certificate_fits shapes
// One LP of any shape on the device (the basis in range without repeats, eps >= 0): the crash on [B | I | b] by the
// single-LP launch pair, B^-1 A, then the reductions; every pointer is a device pointer.  Returns LP_OPTIMAL /
// LP_SINGULAR (outputs untouched).
int lp_basis_certificate_device(lp_context* ctx, const double* dA, int m, int n, const double* db, const double* dc,
                                const int* dbasis, int maximize, double eps, int* dkind, double* dfarkas,
                                double* dray, double* dvalue, int* dindex);

// Parametric right-hand-side paths from given optimal bases, one LP per workgroup (basis_parametric.hip): the
// re-solve's crash on [A | b | d], then one dual-simplex pivot per breakpoint of z*(t) = opt { c.x : A x = b + t d }.
// The parametric cost (below) takes the same struct.
struct BasisParametricDev {
    int batch, m, n;
    int pitch;              // row pitch (doubles) of the LDS tableau: lp_basis_parametric[_cost]_lds_bytes
    int max_breaks;
    int max_iter;           // 0 (batched_lds_loop.hpp's primal loop is compiled in but never called; cost: ignored)
    double eps, t_max;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    const double* dir;      // batch x m: the direction d (cost: batch x n, the cost direction g)
    const int* basis;       // batch x m (by position)
    const int* run_status;  // batch, or nullptr: an LP whose entry is not LP_OPTIMAL keeps it and gets nseg 0
    int* nseg;              // batch
    double* t;              // batch x (max_breaks+2)
    double* obj;            // batch x (max_breaks+2)
    double* slope;          // batch x (max_breaks+1)
    int* enter;             // batch x (max_breaks+1)
    int* leave;             // batch x (max_breaks+1)
    int* basis_out;         // batch x m: the final basis (the given one without a path)
    int* status;            // batch
};

// basis_parametric.hip
size_t lp_basis_parametric_lds_bytes(int m, int n, int* pitch_out);
int lp_basis_parametric_launch(lp_context* ctx, const BasisParametricDev& d, int maximize);   // fitting shapes
// One LP of any shape on the device (the basis in range, eps >= 0, t_max >= 0, max_breaks >= 0): the crash on
// [A | d | b] by the single-LP launch pair, then one selector + rank-1 update pair per breakpoint under the polling
// loop; every pointer is a device pointer.  Returns the path's status (LP_OPTIMAL, LP_INFEASIBLE, LP_ITER_LIMIT:
// nseg, t .. leave written up to the path's end, basis_out the final basis) or LP_SINGULAR / LP_BAD_ARG (outputs
// untouched).
int lp_basis_parametric_device(lp_context* ctx, const double* dA, int m, int n, const double* db, const double* dc,
                               const int* dbasis, const double* ddir, int maximize, double t_max, double eps,
                               int max_breaks, int* dnseg, double* dt, double* dobj, double* dslope, int* denter,
                               int* dleave, int* dbasis_out);

// Parametric cost paths from given optimal bases, one LP per workgroup (basis_parametric_cost.hip): the re-solve's
// crash on [A | b; c | 0; g | 0], then one primal pivot per breakpoint of z*(t) = opt { (c + t g).x : A x = b }.
// It takes a BasisParametricDev whose dir is g.

// basis_parametric_cost.hip
size_t lp_basis_parametric_cost_lds_bytes(int m, int n, int* pitch_out);
int lp_basis_parametric_cost_launch(lp_context* ctx, const BasisParametricDev& d, int maximize);   // fitting shapes
// One LP of any shape on the device (the basis in range, eps >= 0, t_max >= 0, max_breaks >= 0): the crash on
// [A | b; g | 0] and on [A | b; c | 0] by the single-LP launch pair, then one selector + rank-1 update pair over m+2
// rows per breakpoint under the polling loop; every pointer is a device pointer.  Returns the path's status
// (LP_OPTIMAL, LP_UNBOUNDED, LP_ITER_LIMIT: nseg, t .. leave written up to the path's end, basis_out the final basis)
// or LP_SINGULAR / LP_BAD_ARG (outputs untouched).
int lp_basis_parametric_cost_device(lp_context* ctx, const double* dA, int m, int n, const double* db,
                                    const double* dc, const int* dbasis, const double* dg, int maximize, double t_max,
                                    double eps, int max_breaks, int* dnseg, double* dt, double* dobj, double* dslope,
                                    int* denter, int* dleave, int* dbasis_out);

// Depth-first branch-and-bound, one integer LP per workgroup (batched_mip.hip): the re-solve's root, then per node a
// row appended in tableau form (first child) or a crash from A and the path's branch rows (second child).
#define LP_MIP_MAX_DEPTH 64
struct BatchedMipDev {
    int batch, m, n, n_orig;
    int maximize;
    int max_iter;           // per node
    int max_depth, max_nodes;
    double eps, int_tol, gap;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    const int* basis_in;    // batch x m (by position): the root's start
    const int* run_status;  // batch, or nullptr: an LP whose entry is not LP_OPTIMAL keeps it (found 0, NaN outputs)
    const int* integer;     // n: the mask, one for the whole batch
    double* x;              // batch x n_orig: the incumbent, NaN without one
    double* obj;            // batch
    double* bound;          // batch
    int* found;             // batch
    int* stats;             // batch x 4: nodes, dual pivots, primal pivots, deepest level
    int* status;            // batch
};

// batched_mip.hip
size_t lp_mip_lds_bytes(int m, int n, int max_depth);
bool lp_mip_fits_shape(int m, int n, int max_depth);
int lp_batched_mip_launch(lp_context* ctx, const BatchedMipDev& d);   // fitting shapes, else LP_BAD_ARG
// basis_driver.hip: the checks both searches share (the mask, int_tol, gap, max_nodes, max_depth in [0, depth_cap])
int lp_mip_check_search(lp_context* ctx, const char* who, int n, int n_orig, const int* integer, double int_tol,
                        double gap, int max_depth, int depth_cap, int max_nodes);

// A batch of same-shape LPs with variable bounds lo <= x <= hi solved by the two-phase bounded-variable simplex, one LP
// per workgroup (batched_bounded.hip; the definition is tests/ref/bounded_ref.c).
struct BatchedBoundedDev {
    int batch, m, n;        // n = canonical columns (the m artificials are implicit)
    int pitch;              // row pitch (doubles) of the LDS tableau, odd, >= n + 1
    int maximize;
    int max_iter;           // per phase: pivots plus bound flips
    double eps;
    const double* A;        // batch x (m*n), each column-major
    const double* b;        // batch x m
    const double* c;        // batch x n
    const double* lo;       // batch x n, finite
    const double* hi;       // batch x n, finite or +inf
    double* x;              // batch x n  (full vertex; written for LP_OPTIMAL only)
    int* basis_out;         // batch x m  (by position)
    int* at_upper;          // batch x n  (0/1: the column is held complemented)
    int* iters;             // batch x 4  (phase-I pivots, drive-out pivots, phase-II pivots, bound flips)
    int* status;            // batch
};

// batched_bounded.hip
size_t lp_bounded_lds_bytes(int m, int n, int* pitch_out);
bool lp_bounded_fits_shape(int m, int n);
size_t lp_bounded_devex_lds_bytes(int m, int n);                    // the carve with the Devex weights behind it
bool lp_bounded_rule_fits_shape(int m, int n, int pivot_rule);      // a known rule, lp_bounded_fits_shape, Devex: the weights too
// The re-solve under a dual rule too (LP_DUAL_*): one weight region for the loop that runs, n doubles for the primal
// Devex, m for the dual Devex, the larger when both are chosen, none otherwise
inline int lp_bounded_resolve_weights(int m, int n, int pivot_rule, int dual_rule) {
    const int p = pivot_rule == LP_PIVOT_DEVEX ? n : 0, q = dual_rule == LP_DUAL_DEVEX ? m : 0;
    return p > q ? p : q;
}
size_t lp_bounded_weights_lds_bytes(int m, int n, int weights);     // the carve with `weights` doubles behind it
bool lp_bounded_dual_rule_fits_shape(int m, int n, int pivot_rule, int dual_rule);   // known rules, and that carve <= 160 KiB
// fitting shapes (under the rule), else LP_BAD_ARG; LP_PIVOT_DANTZIG launches the kernel there has always been
int lp_batched_bounded_launch(lp_context* ctx, const BatchedBoundedDev& d, int pivot_rule = LP_PIVOT_DANTZIG);

// The same batch re-solved from given bases and complement flags, one LP per workgroup (batched_bounded_resolve.hip;
// the definition is tests/ref/bounded_resolve_ref.c).  max_iter bounds the dual pivots, or the primal pivots plus
// flips; iters is batch x 3 (dual pivots, primal pivots, bound flips).
struct BatchedBoundedResolveDev : BatchedBoundedDev {
    const int* basis_in;     // batch x m (by position), every index in [0, n)
    const int* at_upper_in;  // batch x n (0/1; 1 only where hi is finite)
};

// batched_bounded_resolve.hip
// fitting shapes (under the rule), else LP_BAD_ARG; the rule governs the primal branch only, dual_rule and dual_ratio
// (LP_DUAL_RATIO_*) the dual branch only
int lp_batched_bounded_resolve_launch(lp_context* ctx, const BatchedBoundedResolveDev& d, int pivot_rule = LP_PIVOT_DANTZIG,
                                      int dual_rule = LP_DUAL_DANTZIG, int dual_ratio = LP_DUAL_RATIO_TEXTBOOK);

// Depth-first branch-and-bound over variable bounds, one mixed-integer bounded LP per workgroup
// (batched_mip_bounded.hip; the definition is tests/ref/mip_bounded_ref.c): the bounded re-solve at the root, then per
// node one bound changed on the live tableau (first child) or the re-solve's install from the path's bounds and the
// recorded basis and flags (second child).  The tableau never grows, so the depth is bounded by the records alone.
#define LP_MIP_BOUNDED_MAX_DEPTH 1024
#define LP_MIP_BOUNDED_MAX_SNAPSHOTS 1024   // lp_mip_bounded_solve_large_ex: the tableau snapshots a call may ask for
struct BatchedMipBoundedDev {
    int batch, m, n, n_orig;
    int maximize;
    int max_iter;            // per node: dual pivots, or primal pivots plus flips
    int max_depth, max_nodes;
    double eps, int_tol, gap;
    const double* A;         // batch x (m*n), each column-major
    const double* b;         // batch x m
    const double* c;         // batch x n
    const double* lo;        // batch x n, finite
    const double* hi;        // batch x n, finite or +inf
    const int* basis_in;     // batch x m (by position), every index in [0, n): the root's start
    const int* at_upper_in;  // batch x n (0/1; 1 only where hi is finite)
    const int* root_status;  // batch, or nullptr: an LP whose entry is not LP_OPTIMAL keeps it (found 0, NaN outputs)
    const int* integer;      // n: the mask, one for the whole batch
    double* x;               // batch x n_orig: the incumbent, NaN without one
    double* obj;             // batch
    double* bound;           // batch
    int* found;              // batch
    int* stats;              // batch x 5: nodes, dual pivots, primal pivots, bound flips, deepest level
    int* status;             // batch
};

// batched_mip_bounded.hip
size_t lp_mip_bounded_lds_bytes(int m, int n, int max_depth);
bool lp_mip_bounded_fits_shape(int m, int n, int max_depth);
// fitting shapes, else LP_BAD_ARG; dual_ratio (LP_DUAL_RATIO_*) picks the ratio test of every dual loop of the search:
// LP_DUAL_RATIO_LONG_STEP launches k_batched_mip_bounded_long (tests/ref/mip_bounded_long_step_ref.c), the same LDS
int lp_batched_mip_bounded_launch(lp_context* ctx, const BatchedMipBoundedDev& d, int dual_ratio = LP_DUAL_RATIO_TEXTBOOK);

// The dual solution and RHS / cost ranging of bounded-variable LPs at given bases and at-upper flags, one LP per
// workgroup (basis_bounded.hip; the definition is tests/ref/bounded_sens_ref.c).  The duals launch writes x, y, d, w;
// the ranging launch writes rhs .. cost_var in interleaved pairs (lower end, upper end).
struct BasisBoundedDev {
    int batch, m, n;
    int maximize;            // ranging only
    double eps;              // ranging only
    const double* A;         // batch x (m*n), each column-major
    const double* b;         // batch x m
    const double* c;         // batch x n
    const double* lo;        // batch x n, finite
    const double* hi;        // batch x n, finite or +inf
    const int* basis;        // batch x m (by position), every index in [0, n)
    const int* at_upper;     // batch x n (0/1; 1 only where hi is finite)
    double* x;               // batch x n: the point the basis and the flags define
    double* y;               // batch x m
    double* d;               // batch x n
    double* w;               // batch
    double* rhs;             // batch x 2m
    int* rhs_var;            // batch x 2m: the leaving column at each end
    int* rhs_side;           // batch x 2m: 0 it leaves at its lower bound, 1 at its upper bound
    double* cost;            // batch x 2n
    int* cost_var;           // batch x 2n: the entering column at each end
    int* status;             // batch: LP_OPTIMAL, LP_SINGULAR or LP_INFEASIBLE (crossed bounds)
};

// basis_bounded.hip
size_t lp_basis_bounded_lds_bytes(int m, int n);
bool lp_basis_bounded_fits_shape(int m, int n);   // lp_bounded_fits_shape and the kernel's LDS <= 160 KiB
int lp_basis_bounded_launch(lp_context* ctx, const BasisBoundedDev& d, bool ranging);   // fitting shapes, else LP_BAD_ARG
// One LP of any shape on the device (d.batch = 1; bounds, basis and flags checked by the caller, eps >= 0): the crash
// on [B | I | b'] ([B | b'] for the duals) by the single-LP launch pair, y and d by lp_basis_duals_device, then x and
// w, or B^-1 A and the reductions.  Returns LP_OPTIMAL / LP_INFEASIBLE / LP_SINGULAR (outputs untouched unless
// LP_OPTIMAL); d.status is not written.
int lp_basis_bounded_device(lp_context* ctx, const BasisBoundedDev& d, bool ranging);

// Farkas and unbounded-ray certificates of bounded-variable LPs at given bases and at-upper flags, one LP per
// workgroup (basis_bounded_certificate.hip; the definition is tests/ref/bounded_certificate_ref.c): the ranging crash
// on [B | I | b'] with the artificials' columns, then the case's alpha chains under the box's sign test.
struct BasisBoundedCertificateDev {
    int batch, m, n;
    int maximize;
    double eps;
    const double* A;         // batch x (m*n), each column-major
    const double* b;         // batch x m
    const double* c;         // batch x n
    const double* lo;        // batch x n, finite
    const double* hi;        // batch x n, finite or +inf
    const int* basis;        // batch x m (by position), indices in [0, n+m)
    const int* at_upper;     // batch x n (0/1; 1 only where hi is finite)
    const int* run_status;   // batch, or nullptr: only LPs whose entry is LP_INFEASIBLE / LP_UNBOUNDED get a
                             // certificate, the others keep their entry and get NONE
    int* kind;               // batch: LP_CERT_*
    double* farkas;          // batch x m
    double* ray;             // batch x n
    double* value;           // batch
    int* index;              // batch
    int* status;             // batch
};

// basis_bounded_certificate.hip
size_t lp_basis_bounded_certificate_lds_bytes(int m, int n);
bool lp_basis_bounded_certificate_fits_shape(int m, int n);   // lp_bounded_fits_shape and the kernel's LDS <= 160 KiB
int lp_basis_bounded_certificate_launch(lp_context* ctx, const BasisBoundedCertificateDev& d);   // fitting shapes
// One LP of any shape on the device (d.batch = 1; bounds, flags, eps and the basis' range and repeats checked by the
// caller): the column codes, the held values, b' and b0 by small kernels, the crash on [B | I | b'] with the artificial
// columns explicit by the single-LP launch pair, B^-1 A, then the case and its reductions.  Returns LP_OPTIMAL /
// LP_INFEASIBLE / LP_SINGULAR (outputs untouched unless LP_OPTIMAL); d.run_status is not read, d.status not written.
int lp_basis_bounded_certificate_device(lp_context* ctx, const BasisBoundedCertificateDev& d);

// Parametric right-hand-side and parametric cost paths of bounded-variable LPs from given optimal bases and at-upper
// flags, one LP per workgroup (basis_bounded_parametric.hip; the definition is tests/ref/bounded_parametric_ref.c): the
// bounded re-solve's tableau with one more right-hand column (b + t dir) or one more cost row (c + t dir), then one
// dual pivot, primal pivot or bound flip per breakpoint of z*(t).
struct BasisBoundedParametricDev {
    int batch, m, n;
    int maximize;
    int max_breaks;
    double eps, t_max;
    const double* A;         // batch x (m*n), each column-major
    const double* b;         // batch x m
    const double* c;         // batch x n
    const double* lo;        // batch x n, finite
    const double* hi;        // batch x n, finite or +inf
    const double* dir;       // batch x m (the RHS path's d) or batch x n (the cost path's g)
    const int* basis;        // batch x m (by position), every index in [0, n)
    const int* at_upper;     // batch x n (0/1; 1 only where hi is finite)
    const int* run_status;   // batch, or nullptr: an LP whose entry is not LP_OPTIMAL keeps it and gets nseg 0
    int* nseg;               // batch
    double* t;               // batch x (max_breaks+2)
    double* obj;             // batch x (max_breaks+2)
    double* slope;           // batch x (max_breaks+1)
    int* enter;              // batch x (max_breaks+1)
    int* leave;              // batch x (max_breaks+1)
    int* side;               // batch x (max_breaks+1): 0 leave[k] stops at its lower bound, 1 at its upper bound
    int* basis_out;          // batch x m: the final basis (the given one without a path)
    int* at_upper_out;       // batch x n: the final flags (the given ones without a path)
    int* status;             // batch
};

// basis_bounded_parametric.hip (cost: the cost path's kernel and carve)
size_t lp_basis_bounded_parametric_lds_bytes(int m, int n, bool cost);
bool lp_basis_bounded_parametric_fits_shape(int m, int n, bool cost);   // lp_bounded_fits_shape and the carve <= 160 KiB
int lp_basis_bounded_parametric_launch(lp_context* ctx, const BasisBoundedParametricDev& d, bool cost);   // fitting shapes
// basis_bounded_parametric_large.hip: one LP of any shape on the tableau in HBM (d.batch = 1; the arguments, bounds,
// flags, basis range and crossed bounds checked by the caller; d.run_status is not read, d.status not written).  The
// selectors' dynamic LDS for m rows must not exceed 156 KiB (LP_BAD_ARG with a message, nothing launched).  Returns the
// path's status; *nseg_host > 0 says that a path was written: then d.t, d.obj [0, nseg], d.slope, d.enter, d.leave,
// d.side [0, nseg), d.basis_out and d.at_upper_out hold it and everything else is untouched.  LP_SINGULAR and
// LP_BAD_ARG (the start is not optimal) write nothing.
size_t lp_basis_bounded_parametric_large_lds_bytes(int m, bool cost);
int lp_basis_bounded_parametric_device(lp_context* ctx, const BasisBoundedParametricDev& d, bool cost, int* nseg_host);

// A batch handle of the C ABI (batched_driver.hip: upload, run, download); the analyses of basis_driver.hip read its
// inputs and final bases after a run.  The kind says which kernel a resident handle launches and which single-LP
// entry its per-LP fallback calls; everything else is the same for the three kinds.
enum lp_batched_kind {
    LP_BATCHED_PLAIN,       // lp_batched_upload: from given bases, one pivot count per LP
    LP_BATCHED_TWO_PHASE,   // lp_batched_two_phase_upload: no starting basis; phase I, drive-out, phase II
    LP_BATCHED_RESOLVE      // lp_batched_resolve_upload: re-solved from given bases; dual pivots, primal pivots
};

struct lp_batched_problem {
    lp_context* ctx = nullptr;
    lp_batched_kind kind = LP_BATCHED_PLAIN;
    int batch = 0, m = 0, n = 0, n_orig = 0;
    int maximize = 0;
    int iter_width = 1;                 // pivot counts per LP: 1, 3, 2 (by kind)
    int pivot_rule = LP_PIVOT_DANTZIG;  // lp_batched_set_pivot_rule: read by every run
    bool resident = false;              // true: one LP per workgroup on the GPU; false: per-LP fallback
    bool ran = false;                   // a run completed: the analyses have final bases to read
    std::vector<double> h_c;            // the costs (the objective of download)
    std::vector<int> status, iters;     // of the last run: batch, batch*iter_width (a resident handle's: as of the last download)
    // resident: one device allocation and the pieces carved from it (dbasis_in: not for two-phase batches)
    char* arena = nullptr;
    int pitch = 0;                      // row pitch of the kernel's LDS tableau
    double *dA = nullptr, *db = nullptr, *dc = nullptr, *dx = nullptr;
    int *dbasis_in = nullptr, *dbasis_out = nullptr, *diters = nullptr, *dstatus = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    unsigned long long* dstamps = nullptr;   // BatchedDev::stamps (LP_BATCHED_STAMPS), allocated by the first run
    int stamps_reg = 0;
    // per-LP fallback: the inputs, and what each LP's run left (x and obj of LP_OPTIMAL LPs only)
    std::vector<double> h_A, h_b;
    std::vector<int> h_basis_in;            // batch*m (not for two-phase batches)
    std::vector<lp_simplex_problem*> lps;   // plain batches: the uploaded LPs, kept between runs
    std::vector<double> h_x, h_obj;         // batch*n_orig, batch
    std::vector<int> h_basis;               // batch*m
};
