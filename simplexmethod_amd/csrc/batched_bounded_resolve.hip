// batched_bounded_resolve.hip — many bounded-variable LPs of one shape RE-SOLVED FROM GIVEN BASES AND COMPLEMENT
// FLAGS, ONE LP PER WORKGROUP.
//
// The case of a branch, a fixing or a what-if on an LP that lp_simplex_bounded has solved: under any change of lo, hi
// or b the old optimal basis stays dual feasible, so a few dual pivots replace the two-phase solve.  Each workgroup
// runs tests/ref/bounded_resolve_ref.c for its LP:
//   - the tableau [A | b'; c | 0] of the shifted variables x' = x - lo with every flagged column held complemented
//     (-A_ij, -c_j); b' is one serial fma chain per row, over the columns with lo_j != 0 and then over the flagged ones;
//   - the basis installed by batched_resolve_crash.hpp (skipped for the slack identity with zero costs);
//   - classify: a position is violated below (xB_t < -eps) or above (U finite, U - xB_t < -eps).  None violated: the
//     bounded primal loop (batched_bounded_loop.hpp, phase-II form); else no slot of a variable < n with d > eps (max)
//     / d < -eps (min): the bounded dual loop (batched_bounded_dual_loop.hpp); else LP_BAD_ARG for this LP.
// hi < lo in some column (U_j < 0, see batched_bounded.hip) ends the LP LP_INFEASIBLE before the crash.
//
// Layout and FITS: batched_bounded.hip's (batched_bounded_carve.hpp, lp_simplex_bounded_fits); the basis and the
// flags are read from HBM.  After the crash the lcol buffer holds the row permutation until the rows are in position
// order.  There is no host fallback: larger shapes get LP_BAD_ARG.
// The kernel's text is batched_bounded_resolve_body.hpp, shared with its Bland and Devex forms below, in which the
// rule governs the primal branch only, and with the _ddevex forms, in which the dual branch prices by Devex
// (LP_DUAL_DEVEX) under each of the three primal rules, and with the _long forms of all six, in which the dual branch
// enters by the bound-flipping ratio test (LP_DUAL_RATIO_LONG_STEP).
#include <cfloat>
#include <climits>

#include "device_select.hpp"
#include "lp_internal.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"
#include "batched_bounded_carve.hpp"

namespace {

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve(BatchedBoundedResolveDev d) {
#include "batched_bounded_resolve_body.hpp"
}

// The same kernel under Bland's rule (LP_PIVOT_BLAND) in the primal branch: batched_bounded_loop.hpp's
// smallest-index pricing and its ratio test with the entering variable's own candidate.
template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_bland(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_BLAND
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_BLAND
}

// The same kernel under Devex pricing (LP_PIVOT_DEVEX) in the primal branch: one weight per slot behind the carve (n
// doubles more: lp_bounded_devex_lds_bytes), 1.0 when a loop starts; Dantzig's ratio test, flip and complement.
template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_devex(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_DEVEX
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DEVEX
}

// The three kernels above with Devex pricing in the dual branch (LP_DUAL_DEVEX, batched_bounded_dual_loop.hpp): one
// weight per basis position behind the carve, m doubles, in the region of the primal Devex weights where the kernel
// has both (n >= m doubles then: lp_bounded_resolve_weights).
template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_ddevex(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_DUAL_DEVEX
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_DEVEX
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_bland_ddevex(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_BLAND
#define LP_BOUNDED_DUAL_DEVEX
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_DEVEX
#undef LP_BOUNDED_BLAND
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_devex_ddevex(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_DEVEX
#define LP_BOUNDED_DUAL_DEVEX
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_DEVEX
#undef LP_BOUNDED_DEVEX
}

// The six kernels above with the bound-flipping ratio test in the dual branch (LP_DUAL_RATIO_LONG_STEP,
// batched_bounded_dual_loop.hpp): the same carve, no LDS more.
template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_long(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_DUAL_LONG_STEP
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_LONG_STEP
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_ddevex_long(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_DUAL_DEVEX
#define LP_BOUNDED_DUAL_LONG_STEP
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_LONG_STEP
#undef LP_BOUNDED_DUAL_DEVEX
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_bland_long(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_BLAND
#define LP_BOUNDED_DUAL_LONG_STEP
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_LONG_STEP
#undef LP_BOUNDED_BLAND
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_bland_ddevex_long(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_BLAND
#define LP_BOUNDED_DUAL_DEVEX
#define LP_BOUNDED_DUAL_LONG_STEP
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_LONG_STEP
#undef LP_BOUNDED_DUAL_DEVEX
#undef LP_BOUNDED_BLAND
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_devex_long(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_DEVEX
#define LP_BOUNDED_DUAL_LONG_STEP
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_LONG_STEP
#undef LP_BOUNDED_DEVEX
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded_resolve_devex_ddevex_long(BatchedBoundedResolveDev d) {
#define LP_BOUNDED_DEVEX
#define LP_BOUNDED_DUAL_DEVEX
#define LP_BOUNDED_DUAL_LONG_STEP
#include "batched_bounded_resolve_body.hpp"
#undef LP_BOUNDED_DUAL_LONG_STEP
#undef LP_BOUNDED_DUAL_DEVEX
#undef LP_BOUNDED_DEVEX
}

}  // namespace

int lp_batched_bounded_resolve_launch(lp_context* ctx, const BatchedBoundedResolveDev& d, int pivot_rule, int dual_rule,
                                      int dual_ratio) {
    if (!lp_pivot_rule_known(pivot_rule)) LP_FAIL(ctx, LP_BAD_ARG, "batched bounded re-solve: unknown pivot rule");
    if (!lp_dual_rule_known(dual_rule)) LP_FAIL(ctx, LP_BAD_ARG, "batched bounded re-solve: unknown dual rule");
    if (!lp_dual_ratio_known(dual_ratio)) LP_FAIL(ctx, LP_BAD_ARG, "batched bounded re-solve: unknown dual ratio test");
    if (dual_ratio == LP_DUAL_RATIO_LONG_STEP) {   // the carve of the textbook kernel under the same two rules
        if (!lp_bounded_dual_rule_fits_shape(d.m, d.n, pivot_rule, dual_rule))
            LP_FAIL(ctx, LP_BAD_ARG, "batched bounded re-solve, long-step: the tableau and the weights do not fit one CU's LDS (lp_simplex_bounded_dual_rule_fits)");
        const size_t cells = (size_t)(d.m + 1) * (d.n + 1);
        const size_t lds = lp_bounded_weights_lds_bytes(d.m, d.n, lp_bounded_resolve_weights(d.m, d.n, pivot_rule, dual_rule));
        const bool dd = dual_rule == LP_DUAL_DEVEX;
        if (pivot_rule == LP_PIVOT_DEVEX)
            return dd ? lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_devex_ddevex_long<256>,
                                         k_batched_bounded_resolve_devex_ddevex_long<1024>, lds, d)
                      : lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_devex_long<256>,
                                         k_batched_bounded_resolve_devex_long<1024>, lds, d);
        if (pivot_rule == LP_PIVOT_BLAND)
            return dd ? lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_bland_ddevex_long<256>,
                                         k_batched_bounded_resolve_bland_ddevex_long<1024>, lds, d)
                      : lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_bland_long<256>,
                                         k_batched_bounded_resolve_bland_long<1024>, lds, d);
        return dd ? lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_ddevex_long<256>,
                                     k_batched_bounded_resolve_ddevex_long<1024>, lds, d)
                  : lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_long<256>, k_batched_bounded_resolve_long<1024>,
                                     lds, d);
    }
    if (dual_rule == LP_DUAL_DEVEX) {
        if (!lp_bounded_dual_rule_fits_shape(d.m, d.n, pivot_rule, dual_rule))
            LP_FAIL(ctx, LP_BAD_ARG, "batched bounded re-solve, dual Devex: the tableau and the weights do not fit one CU's LDS (lp_simplex_bounded_dual_rule_fits)");
        const size_t cells = (size_t)(d.m + 1) * (d.n + 1);
        const size_t lds = lp_bounded_weights_lds_bytes(d.m, d.n, lp_bounded_resolve_weights(d.m, d.n, pivot_rule, dual_rule));
        if (pivot_rule == LP_PIVOT_DEVEX)
            return lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_devex_ddevex<256>,
                                    k_batched_bounded_resolve_devex_ddevex<1024>, lds, d);
        if (pivot_rule == LP_PIVOT_BLAND)
            return lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_bland_ddevex<256>,
                                    k_batched_bounded_resolve_bland_ddevex<1024>, lds, d);
        return lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_ddevex<256>, k_batched_bounded_resolve_ddevex<1024>,
                                lds, d);
    }
    if (!lp_bounded_fits_shape(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "batched bounded re-solve: the shape does not fit one CU's LDS");
    if (!lp_bounded_rule_fits_shape(d.m, d.n, pivot_rule))
        LP_FAIL(ctx, LP_BAD_ARG, "batched bounded re-solve, Devex: the tableau and the weights do not fit one CU's LDS (lp_simplex_bounded_rule_fits)");
    const size_t cells = (size_t)(d.m + 1) * (d.n + 1);
    if (pivot_rule == LP_PIVOT_DEVEX)
        return lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_devex<256>, k_batched_bounded_resolve_devex<1024>,
                                lp_bounded_devex_lds_bytes(d.m, d.n), d);
    if (pivot_rule == LP_PIVOT_BLAND)
        return lp_launch_per_lp(ctx, cells, k_batched_bounded_resolve_bland<256>, k_batched_bounded_resolve_bland<1024>,
                                lp_bounded_lds_bytes(d.m, d.n, nullptr), d);
    return lp_launch_per_lp(ctx, (size_t)(d.m + 1) * (d.n + 1), k_batched_bounded_resolve<256>,
                            k_batched_bounded_resolve<1024>, lp_bounded_lds_bytes(d.m, d.n, nullptr), d);
}
