// batched_resolve.hip — many LPs of one shape RE-SOLVED FROM GIVEN BASES, ONE LP PER WORKGROUP.
//
// The case of a branch-and-bound or parametric loop: the old optimal basis of an LP whose right-hand side
// changed stays dual feasible (the reduced costs do not depend on b) but may be primal infeasible.  Each
// workgroup re-solves one LP exactly as tests/ref/resolve_ref.c states it:
//   - install the basis: orc_simplex_tableau's crash (skipped for the slack identity with zero costs): for
//     t = 0 .. m-1 a forced pivot of column N(t) on the first-max |T[i][N(t)]| over the rows still held by an
//     artificial, the singular verdict minp <= DBL_EPSILON*m*maxp, then the rows permuted in place into
//     basis-position order (cycle by cycle through the prow buffer);
//   - classify: no xB_t < -eps -> the primal loop (batched_lds_loop.hpp with the artificial slots barred, as in
//     the two-phase kernel's phase II: Dantzig, pricing keyed by variable index, ratio test keyed by position); else no non-basic d_j > eps (max) /
//     d_j < -eps (min) -> the dual loop; else LP_BAD_ARG (the basis is no valid start);
//   - dual loop: the leaving position is the EPS-hysteresis chain (min) over xB_t with xB_t < -eps, in
//     position order (none: optimal); the entering variable the same chain over q_j = d_j / T[r][j] (max) or
//     -d_j / T[r][j] (min) of the non-basic j with T[r][j] < -eps, in variable-index order (none: infeasible).
//
// Layout: batched_two_phase.hip's (the same LDS bytes and FITS predicate).  The tableau starts as [A | b]
// with the m artificial columns of its identity implicit: every original column has a slot, and a crash
// pivot leaves the artificial's column in the entering variable's slot, barred from then on.  After the
// crash the lcol buffer holds the row permutation (ints) until the rows are in position order.
#include <cfloat>

#include "device_select.hpp"
#include "lp_internal.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"

namespace {

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_resolve(BatchedResolveDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int m = d.m, n = d.n, W = n + 1, pitch = d.pitch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve (batched_two_phase.hip)
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = smem + sizeof(Published) / 8;             // (m+1) x pitch
    double* prow = T + (size_t)(m + 1) * pitch;           // W
    double* lcol = prow + W;                              // m+1
    int* slotvar = reinterpret_cast<int*>(lcol + m + 1);  // n
    int* basis = slotvar + n;                             // m
    int* pub = pubs->v;   // [0] entering slot / crash row, [1] leaving position, [2] singular verdict, [3] block_any

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const int* N = d.basis_in + (size_t)lp * m;
    const double eps = d.eps;
    const bool maximize = d.maximize != 0;
    constexpr int ANY_WORD = 3;   // block_any's word of pub
#include "batched_block_any.hpp"

    // ---- T = [A | b; c | 0]; slots = the columns in order, basis = the artificials by row
    for (int s = tid; s < n; s += NT) slotvar[s] = s;
    for (int t = tid; t < m; t += NT) basis[t] = n + t;
    for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
        const int s = e / m, i = e - s * m;
        T[(size_t)i * pitch + s] = A[e];
    }
    for (int i = tid; i < m; i += NT) T[(size_t)i * pitch + n] = b[i];
    for (int j = tid; j < W; j += NT) T[(size_t)m * pitch + j] = (j < n) ? c[j] : 0.0;
    // the crash is skipped when the basis columns are the unit vectors in order and their costs are zero
    int not_identity = 0;
    for (int e = tid; e < m * m; e += NT) {
        const int t = e / m, i = e - t * m;
        if (A[(size_t)N[t] * m + i] != ((i == t) ? 1.0 : 0.0)) not_identity = 1;
    }
    for (int t = tid; t < m; t += NT)
        if (c[N[t]] != 0.0) not_identity = 1;
    const bool identity = !block_any(not_identity);

    // ---- pivot(r, se) and the primal loop simplex(phase2, maximize, iters) (Dantzig's rule)
    constexpr bool BLAND = false;
#include "batched_lds_loop.hpp"

    int status = LP_OPTIMAL;
#include "batched_resolve_crash.hpp"

    // ---- the dual loop: leaving position, then entering slot, both chains by wave 0
#include "batched_dual_loop.hpp"

    int it[2] = {0, 0};   // dual pivots, primal pivots
    if (status == LP_OPTIMAL) {
        // ---- classification: two block reductions over the crashed tableau
        const double* drow = T + (size_t)m * pitch;
#include "batched_resolve_classify.hpp"
        if (primal_feasible)
            status = simplex(true, maximize, it[1]);   // phase II's form: artificial slots barred
        else if (dual_feasible)
            status = dual(it[0]);
        else
            status = LP_BAD_ARG;
        __syncthreads();
    }
    // ---- outputs: x(N(t)) = xB(t), zeros elsewhere; the basis by position (the given one when singular)
    double* x = d.x + (size_t)lp * n;
    for (int j = tid; j < n; j += NT) x[j] = 0.0;
    __syncthreads();
    for (int t = tid; t < m; t += NT) {
        const bool given = status == LP_SINGULAR;
        if (!given && basis[t] < n) x[basis[t]] = T[(size_t)t * pitch + n];
        d.basis_out[(size_t)lp * m + t] = given ? N[t] : basis[t];
    }
    if (tid == 0) {
        d.iters[(size_t)lp * 2 + 0] = it[0];
        d.iters[(size_t)lp * 2 + 1] = it[1];
        d.status[lp] = status;
    }
}

}  // namespace

int lp_batched_resolve_launch(lp_context* ctx, const BatchedResolveDev& d) {
    if (!lp_batched_two_phase_fits(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "batched re-solve: the shape does not fit one CU's LDS");
    return lp_launch_per_lp(ctx, (size_t)(d.m + 1) * (d.n + 1), k_batched_resolve<256>, k_batched_resolve<1024>,
                            lp_batched_two_phase_lds_bytes(d.m, d.n, nullptr), d);
}
