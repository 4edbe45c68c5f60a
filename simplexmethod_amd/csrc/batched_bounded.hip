// batched_bounded.hip — the two-phase BOUNDED-VARIABLE simplex for many LPs of one shape, ONE LP PER WORKGROUP.
//
// Problem: opt c.x, A x = b, lo <= x <= hi (lo finite, hi finite or +inf).  Each workgroup runs tests/ref/bounded_ref.c
// for its LP: the two-phase flow of batched_two_phase.hip on the shifted variables x' = x - lo in [0, U], U = hi - lo,
// with the upper bounds handled in the ratio test (a bound flip or a complemented leaving variable) rather than by
// rows, so the tableau stays (m+1) x (n+1).  HBM is read once for A, b, c, lo and hi and written once for the results.
// Layout (LDS, doubles unless noted):
//
//   T      (m+1) x pitch   condensed tableau: the n slots, xB (slot n), the reduced-cost row (row m)
//   prow   n+1             pivot row before scaling; v_j (the tableau value of each variable) at the end
//   lcol   m+1             eta column; the rows' sign changes; the phase-II basic costs
//   U, lov n, n            hi - lo and lo per structural column
//   slotvar n, basis m, up n  (ints) variable held by each slot, basic variable by position, complemented flags
//
// The shift b'_i = b_i - sum_{j: lo_j != 0} A_ij lo_j is one serial fma chain per row over the loaded tableau.  hi < lo
// in some column is seen as U_j < 0 (hi - lo < 0 iff hi < lo: subtraction of doubles with gradual underflow is exact
// in sign) and ends the LP LP_INFEASIBLE before any pivot.  The phase steps, the drive-out and the phase-II pricing are
// batched_two_phase_body.hpp's with the phase-II costs sign-changed for complemented columns; the loop is
// batched_bounded_loop.hpp on batched_lds_loop.hpp's pivot.
// The kernel's text is batched_bounded_body.hpp, shared with its Bland and Devex forms below.
//
// FITS (lp_simplex_bounded_fits): lp_bounded_lds_bytes(m, n) <= 160 KB, one CU's LDS.  Canonical 64 x 192 takes 105 KB.
// There is no host fallback: larger shapes get LP_BAD_ARG.  Under LP_PIVOT_DEVEX the carve carries n more doubles, the
// weights (lp_simplex_bounded_rule_fits); the Dantzig kernel is the one lp_simplex_bounded has always launched.
#include <climits>

#include "device_select.hpp"
#include "lp_internal.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"
#include "batched_bounded_carve.hpp"

namespace {

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded(BatchedBoundedDev d) {
#include "batched_bounded_body.hpp"
}

// The same kernel under Bland's rule (LP_PIVOT_BLAND) in phase I and phase II: batched_bounded_loop.hpp's
// smallest-index pricing and its ratio test with the entering variable's own candidate.
template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_bland(BatchedBoundedDev d) {
#define LP_BOUNDED_BLAND
#include "batched_bounded_body.hpp"
#undef LP_BOUNDED_BLAND
}

// The same kernel under Devex pricing (LP_PIVOT_DEVEX) in phase I and phase II: one weight per slot behind the carve (n
// doubles more: lp_bounded_devex_lds_bytes), 1.0 when a loop starts; Dantzig's ratio test, flip and complement.
template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_devex(BatchedBoundedDev d) {
#define LP_BOUNDED_DEVEX
#include "batched_bounded_body.hpp"
#undef LP_BOUNDED_DEVEX
}

}  // namespace

size_t lp_bounded_lds_bytes(int m, int n, int* pitch_out) {
    const BoundedCarve k = bounded_carve(m, n);
    if (pitch_out) *pitch_out = k.pitch;
    return k.bytes;
}

bool lp_bounded_fits_shape(int m, int n) {
    return m > 0 && n >= m && lp_bounded_lds_bytes(m, n, nullptr) <= 160 * 1024;
}

size_t lp_bounded_devex_lds_bytes(int m, int n) { return bounded_carve(m, n, true).bytes; }

// (the region's size alone decides the bytes: n doubles as `weights` or as `dual_weights` carve alike)
size_t lp_bounded_weights_lds_bytes(int m, int n, int weights) { return bounded_carve(m, n, false, weights).bytes; }

bool lp_bounded_dual_rule_fits_shape(int m, int n, int pivot_rule, int dual_rule) {
    if (!lp_pivot_rule_known(pivot_rule) || !lp_dual_rule_known(dual_rule) || !lp_bounded_fits_shape(m, n)) return false;
    return lp_bounded_weights_lds_bytes(m, n, lp_bounded_resolve_weights(m, n, pivot_rule, dual_rule)) <= 160 * 1024;
}

bool lp_bounded_rule_fits_shape(int m, int n, int pivot_rule) {
    return lp_pivot_rule_known(pivot_rule) && lp_bounded_fits_shape(m, n) &&
           (pivot_rule != LP_PIVOT_DEVEX || lp_bounded_devex_lds_bytes(m, n) <= 160 * 1024);
}

int lp_batched_bounded_launch(lp_context* ctx, const BatchedBoundedDev& d, int pivot_rule) {
    if (!lp_pivot_rule_known(pivot_rule)) LP_FAIL(ctx, LP_BAD_ARG, "batched bounded simplex: unknown pivot rule");
    if (!lp_bounded_fits_shape(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "batched bounded simplex: the shape does not fit one CU's LDS");
    if (!lp_bounded_rule_fits_shape(d.m, d.n, pivot_rule))
        LP_FAIL(ctx, LP_BAD_ARG, "batched bounded simplex, Devex: the tableau and the weights do not fit one CU's LDS (lp_simplex_bounded_rule_fits)");
    const size_t cells = (size_t)(d.m + 1) * (d.n + 1);
    if (pivot_rule == LP_PIVOT_DEVEX)
        return lp_launch_per_lp(ctx, cells, k_batched_bounded_devex<256>, k_batched_bounded_devex<1024>,
                                lp_bounded_devex_lds_bytes(d.m, d.n), d);
    if (pivot_rule == LP_PIVOT_BLAND)
        return lp_launch_per_lp(ctx, cells, k_batched_bounded_bland<256>, k_batched_bounded_bland<1024>,
                                lp_bounded_lds_bytes(d.m, d.n, nullptr), d);
    return lp_launch_per_lp(ctx, (size_t)(d.m + 1) * (d.n + 1), k_batched_bounded<256>, k_batched_bounded<1024>,
                            lp_bounded_lds_bytes(d.m, d.n, nullptr), d);
}
