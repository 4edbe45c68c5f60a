// batched_two_phase.hip — many LPs of one shape WITHOUT a starting basis, ONE LP PER WORKGROUP.
//
// Each workgroup runs the whole two-phase flow of oracle/lp_oracle.c: orc_two_phase for its LP:
// HBM is touched once to load [A | b | c] and once to store the results.  Layout (LDS, doubles):
//
//   T     (m+1) x pitch   condensed tableau: the n slots, xB (slot n), the reduced-cost row (row m)
//   prow  n+1             pivot row before scaling
//   lcol  m+1             eta column (entry m: reduced-cost row); scratch of the infeasibility sum
//   slotvar n, basis m    (ints) variable held by each slot, basic variable by position
//
// The phase-I problem [A' | I] has m artificial columns whose identity is the starting basis, so
// every original column starts non-basic and the condensed tableau is (m+1) x (n+1).  A pivot
// overwrites the entering column's slot with the column of the variable that leaves (exactly what
// tableau_pivot gives that column), so an artificial that leaves keeps a slot and may enter again
// in phase I.  The order-sensitive steps, each with the oracle's arithmetic:
//   - auxiliary problem: rows with b[i] < -eps change sign;
//   - phase-I reduced costs: the crash of orc_simplex_tableau with unit pivots and costs 1, i.e.
//     for every column the serial chain d = fma(-1, A'[t][j], d), t = 0 .. m-1 in row order;
//   - pricing and ratio test: the EPS-hysteresis scans on (value, key) pairs of batched_scan.hpp
//     (key = variable index, resp. basis position); max_iter applies to each phase on its own;
//   - infeasibility: the artificials' values summed in ARTIFICIAL-INDEX order (0 if non-basic);
//   - drive-out: positions in ascending order whose variable is an artificial; for each, the
//     non-basic original column of SMALLEST VARIABLE INDEX with |T[pos][j]| > eps (a min-key
//     reduction over the slots), pivoted before the next position is searched;
//   - phase-II costs: row m reset to c (0 for artificials and xB), then priced out over the basis
//     in POSITION order: d = fma(-c[N(t)] / 1, T[t][j], d) (lp_simplex_phase2_costs' arithmetic);
//     artificial slots are never eligible again.
//
// FITS (the one predicate, lp_batched_two_phase_fits): lp_batched_two_phase_lds_bytes(m, n) <= 160 KB,
// one CU's LDS.  Canonical 64 x 192 takes 104 KB.  Batches of shapes beyond it are solved by the
// host with lp_simplex_two_phase, one LP after another (batched_driver.hip).
#include "device_select.hpp"
#include "lp_internal.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"

namespace {

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_two_phase(BatchedTwoPhaseDev d) {
    constexpr bool BLAND = false;
#include "batched_two_phase_body.hpp"
}

// The same kernel under Bland's rule (LP_PIVOT_BLAND) in phase I and phase II: batched_scan.hpp's keyed
// selections (keys: the variable index for pricing, the basic variable's index for the ratio test).  The
// drive-out is the same under both rules.
template <int NT>
__global__ __launch_bounds__(NT) void k_batched_two_phase_bland(BatchedTwoPhaseDev d) {
    constexpr bool BLAND = true;
#include "batched_two_phase_body.hpp"
}

// The same kernel under Devex pricing (LP_PIVOT_DEVEX) in phase I and phase II: one weight per slot behind the
// carve (n doubles more: lp_batched_two_phase_devex_lds_bytes), set to 1.0 when each phase starts; pricing on
// d * d / w (batched_scan.hpp: wave_argmax_keyed), Dantzig's ratio test, and the weight update by wave 0 before
// the pivot.  The drive-out is the same under every rule and leaves the weights alone.
template <int NT>
__global__ __launch_bounds__(NT) void k_batched_two_phase_devex(BatchedTwoPhaseDev d) {
    constexpr bool BLAND = false;
#define LP_BATCHED_DEVEX
#include "batched_two_phase_body.hpp"
#undef LP_BATCHED_DEVEX
}

}  // namespace

size_t lp_batched_two_phase_lds_bytes(int m, int n, int* pitch_out) {
    const int W = n + 1;
    const int pitch = (W & 1) ? W : W + 1;   // odd pitch: conflict-free column reads
    if (pitch_out) *pitch_out = pitch;
    const size_t dbl = sizeof(Published) / 8 + (size_t)(m + 1) * pitch + W + (m + 1);
    const size_t bytes = dbl * 8 + sizeof(int) * ((size_t)n + m);
    return (bytes + 15) & ~(size_t)15;
}

size_t lp_batched_two_phase_devex_lds_bytes(int m, int n) {
    // (the carve's ints end on a 4-byte boundary when n + m is odd; its size is rounded up to 16, which holds the pad)
    return lp_batched_two_phase_lds_bytes(m, n, nullptr) + (((sizeof(double) * (size_t)n) + 15) & ~(size_t)15);
}

bool lp_batched_two_phase_fits(int m, int n) {
    return m > 0 && n >= m && lp_batched_two_phase_lds_bytes(m, n, nullptr) <= 160 * 1024;
}

int lp_batched_two_phase_launch(lp_context* ctx, const BatchedTwoPhaseDev& d, int pivot_rule) {
    if (!lp_batched_two_phase_fits(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "batched two-phase: the shape does not fit one CU's LDS");
    if (pivot_rule == LP_PIVOT_DEVEX && lp_batched_two_phase_devex_lds_bytes(d.m, d.n) > 160 * 1024)
        LP_FAIL(ctx, LP_BAD_ARG, "batched two-phase Devex: the tableau and the weights do not fit one CU's LDS (lp_batched_devex_fits)");
    const size_t cells = (size_t)(d.m + 1) * (d.n + 1);
    if (pivot_rule == LP_PIVOT_DEVEX)
        return lp_launch_per_lp(ctx, cells, k_batched_two_phase_devex<256>, k_batched_two_phase_devex<1024>,
                                lp_batched_two_phase_devex_lds_bytes(d.m, d.n), d);
    const size_t shm = lp_batched_two_phase_lds_bytes(d.m, d.n, nullptr);
    if (pivot_rule == LP_PIVOT_BLAND)
        return lp_launch_per_lp(ctx, cells, k_batched_two_phase_bland<256>, k_batched_two_phase_bland<1024>, shm, d);
    return lp_launch_per_lp(ctx, cells, k_batched_two_phase<256>, k_batched_two_phase<1024>, shm, d);
}
