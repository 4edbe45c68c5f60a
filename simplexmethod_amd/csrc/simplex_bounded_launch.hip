// simplex_bounded_launch.hip — the bounded-variable simplex on the HBM tableau of simplex_launch.hip
// (lp_simplex_bounded_large, and lp_simplex_bounded_resolve_large's classification and dual loop): one select + one
// rank-1-update launch per iteration, at any shape the launch pair runs.
//
// The definition is tests/ref/bounded_ref.c, which is stated on a condensed slot tableau.  Here the tableau is the full
// one of SimplexDev: (m+1) x ld row-major, one column per variable (the m artificials are columns n_lp .. n_lp+m-1 of
// the phase-I problem, so d.n = n_lp + m), xB in column d.n, row m the reduced costs.  The reference's slot of the
// entering variable receives the eta column; on the full tableau that is the leaving variable's own column after the
// update, fma(l_i, 1, 0) = l_i, because a basic column is the exact unit vector.  Every other entry goes through the
// same operations in the same order, so the results are the reference's bit for bit.
//
// Beside the tableau (BoundedLargeDev, kept out of SimplexDev and SimplexState so that the kernels of
// simplex_launch.hip are what they were):
//   U[d.n]   hi - lo per variable, +inf for the artificials;
//   up[d.n]  1 = the tableau holds U_j - x'_j in place of x'_j (what at_upper_out reports);
//   flips    bound flips since the start of the solve (both phases);
//   q[ld]    scratch of the dual selector: the quotients of its ratio test;
//   w[d.n]   the Devex weights (LP_PIVOT_DEVEX only; the other selectors never touch them).  The dual loop under
//            LP_DUAL_DEVEX keeps its own in the first m of them, one per basis position (a call runs one of the loops).
// SimplexState::iters counts the pivots plus flips of the running phase, which is what max_iter bounds.
//
// A bound flip is done inside the selector (two strided columns, O(m)) and leaves pivot_valid = 0, so the
// k_simplex_update queued behind it returns at once: a flip streams no tableau.  A pivot is staged for the unchanged
// k_simplex_update; when the leaving variable leaves at its upper bound (a_r < -eps) the staged pivot row is the
// complemented one (negated over the columns, xB_r = U - xB_r, the leaving variable's own entry +1 again), and since
// the update writes row r from the staged copy alone, row r of the tableau itself need not be touched first.
//
// The re-solve from a basis (tests/ref/bounded_resolve_ref.c) has no artificial columns: d.n = n_lp, the basis is
// installed by lp_simplex_upload's crash.  k_simplex_classify_bounded picks its loop; the dual loop is
// k_simplex_select_dual_bounded + k_simplex_update per pivot.  There the complement happens BEFORE the ratio test (a
// basic variable above its upper bound is held as U - x, which is below 0, and leaves at that bound), and again only
// the staged pivot row carries it.
//
// Plain C++ and vector stores only: no inline assembly and no scalar-memory writes in this file.
#include "device_select.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kRunning = -100;  // SimplexState::status while pivoting

// Launch shape and LDS as k_simplex_select (u[m+1], ratio[m], 3 ints) plus one double, the selected ratio theta.
__global__ __launch_bounds__(1024) void k_simplex_select_bounded(SimplexDev d, BoundedLargeDev bd) {
    SimplexState* st = d.state;
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_u = s_dyn;
    double* s_ratio = s_dyn + (d.m + 2);
    double& s_theta = s_dyn[2 * (d.m + 2)];
    int* s_int = reinterpret_cast<int*>(s_dyn + 2 * (d.m + 2) + 2);
    int& s_enter = s_int[0];
    int& s_leave = s_int[1];

    const int tid = threadIdx.x;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = d.m, n = d.n, ld = d.ld;
    const double eps = st->eps;
    if (st->iters >= st->max_iter) {   // pivots plus flips of this phase
        if (tid == 0) {
            st->status = LP_ITER_LIMIT;
            st->pivot_valid = 0;
        }
        return;
    }
    // pricing: k_simplex_select's (phase II: the artificial columns carry no non-basic flag)
    const double* drow = d.T + (size_t)m * ld;
    if (tid < 64) {
        double best;
        int e;
        auto load = [&](int j, bool& ok) {
            ok = d.nonbasic[j] != 0;
            return drow[j];
        };
        if (d.maximize)
            e = lpdev::wave_chain_select<true>(n, eps, best, load);
        else
            e = lpdev::wave_chain_select<false>(n, eps, best, load);
        const bool optimal = d.maximize ? (best <= eps) : (best >= -eps);
        if (tid == 0) s_enter = optimal ? -1 : e;
    }
    __syncthreads();
    const int e = s_enter;
    if (e < 0) {
        if (tid == 0) {
            st->status = LP_OPTIMAL;
            st->pivot_valid = 0;
        }
        return;
    }
    // column e, and per basis position the step at which its variable reaches 0 (a > eps) or its upper bound
    // (a < -eps, U finite)
    for (int i = tid; i <= m; i += blockDim.x) {
        const double a = d.T[(size_t)i * ld + e];
        s_u[i] = a;
        if (i < m) {
            const double xb = d.T[(size_t)i * ld + n], u = bd.U[d.basis[i]];
            s_ratio[i] = (a > eps) ? xb / a : (a < -eps && u < INFINITY) ? (xb - u) / a : INFINITY;
        }
    }
    __syncthreads();
    if (tid < 64) {
        double theta;
        auto load = [&](int i, bool& ok) {
            ok = true;  // ineligible rows hold +inf, which the < scan never takes
            return s_ratio[i];
        };
        const int r = lpdev::wave_chain_select<false>(m, eps, theta, load);
        if (tid == 0) {
            s_leave = r;
            s_theta = theta;
        }
    }
    __syncthreads();
    const int r = s_leave;
    const double ue = bd.U[e];
    if (r < 0 && !(ue < INFINITY)) {
        if (tid == 0) {
            st->status = LP_UNBOUNDED;
            st->pivot_valid = 0;
        }
        return;
    }
    if (r < 0 || ue <= s_theta) {   // bound flip: e goes to its other bound, the basis stays
        for (int i = tid; i <= m; i += blockDim.x) {
            const size_t row = (size_t)i * ld;
            d.T[row + n] = fma(-ue, s_u[i], d.T[row + n]);
            d.T[row + e] = -s_u[i];
        }
        if (tid == 0) {
            bd.up[e] ^= 1;
            *bd.flips += 1;
            st->iters += 1;
            st->pivot_valid = 0;
        }
        return;
    }
    // pivot on row r; a_r < -eps: the leaving variable leaves at its upper bound and is complemented first
    const int old = d.basis[r];   // (every thread reads it before the barrier below; thread 0 writes it after)
    const bool comp = s_u[r] < -eps;
    const double ur = comp ? -s_u[r] : s_u[r];
    for (int i = tid; i <= m; i += blockDim.x)
        d.lcol[i] = (i == r) ? 1.0 / ur : -s_u[i] / ur;
    const double* trow = d.T + (size_t)r * ld;
    const double uold = bd.U[old];
    for (int j = tid; j < ld; j += blockDim.x) {
        double v = trow[j];
        if (comp) v = (j < n) ? -v : (j == n) ? uold - v : v;
        if (j == old) v = 1.0;   // the leaving variable's own column: the unit column again (a no-op without comp)
        d.prow[j] = v;
    }
    __syncthreads();
    if (tid == 0) {
        if (comp) bd.up[old] ^= 1;
        d.basis[r] = e;
        d.nonbasic[e] = 0;
        d.nonbasic[old] = 1;
        st->iters += 1;
        st->enter = e;
        st->leave = r;
        st->pivot_valid = 1;
    }
}

// ---------------------------------------------------------------------------
// The bounded selector under a pivot rule (tests/ref/bounded_rules_ref.c is the definition; lp_simplex_bounded_large_ex
// and the primal branch of lp_simplex_bounded_resolve_large_ex).  Launch shape, staging contract and the
// flip-in-selector design are k_simplex_select_bounded's: a flip leaves pivot_valid = 0, a pivot whose leaving variable
// leaves at its upper bound is staged complemented, and up, flips and iters are kept the same way.  Every loop is
// strided over the 1024 threads (m may exceed them, n may exceed one pricing step).
//
// BLAND (k_simplex_select_bounded_bland)
//   entering: the smallest non-basic j with d_j beyond eps, the first-hit scan of k_simplex_select_bland (in phase II
//             the artificial columns carry no non-basic flag);
//   rows:     v_t = xB/a for a > eps, (xB - U)/a for a < -eps with U of basis[t] finite, NaN otherwise (neither the
//             minimum nor the tie test takes a NaN);
//   step:     theta* = min(min_t v_t, U_e), an exact minimum without eps hysteresis; not below +inf: LP_UNBOUNDED;
//   blocking: the rows with v_t <= theta* + eps keyed by basis[t], and the entering variable keyed by e when
//             U_e <= theta* + eps.  The keys are distinct variable indices, so the smallest key is one candidate:
//             e means the bound flip, a row the pivot (complemented first when a_r < -eps).
//
// DEVEX (k_simplex_select_bounded_devex)
//   weights:  bd.w, one per tableau column (d.n of them, the artificial columns included), all exactly 1.0 when a
//             primal loop starts (the host resets them on the stream); the drive-out never touches them;
//   entering: the arg-max of (d_j * d_j) / w_j over the eligible non-basic columns by the whole workgroup, exact ties
//             to the smallest j, a NaN score never taken: the pricing of k_simplex_select_devex;
//   ratio test, flip decision and complement: k_simplex_select_bounded's.  A flip leaves every weight alone;
//   update:   inside the loop that stages prow, from the STAGED row (after the complement, if any), the old
//             u_r (after the complement) and the old w_e: w_j = fmax(w_j, (t * t) * w_e), t = prow_j / u_r, for
//             every j < d.n other than e and the leaving variable v = basis[r]; then w_v = fmax(w_e / (u_r * u_r), 1.0).
//             No multiply feeds an add in the score or the weights, so nothing there can be fused.
//   The reference keeps a weight per slot of its condensed tableau, and the slot of the entering variable passes to
//   the leaving one: on the full tableau that is the weight of the leaving variable's column, w_v.  A basic column
//   j != v holds +0 or -0 in row r; the complement turns that into -0 or +0, still a zero, so t * t = 0 and fmax
//   keeps w_j (and drops the NaN of 0 * inf).  Column v itself holds +1 in row r (-1 before the staging puts the unit
//   entry back in a complemented row) and is skipped.  No weight of a basic column is ever read: a column's weight
//   is rewritten when it leaves the basis, before it can be priced.
// LDS: k_simplex_select_bounded's; Devex adds the sixteen wave results (16 doubles + 16 ints).
// ---------------------------------------------------------------------------
template <int RULE>
__device__ __forceinline__ void select_bounded_rule(const SimplexDev& d, const BoundedLargeDev& bd) {
    SimplexState* st = d.state;
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_u = s_dyn;
    double* s_ratio = s_dyn + (d.m + 2);
    double& s_theta = s_dyn[2 * (d.m + 2)];
    int* s_int = reinterpret_cast<int*>(s_dyn + 2 * (d.m + 2) + 2);
    int& s_enter = s_int[0];
    int& s_leave = s_int[1];   // Bland: -2 = the entering variable blocks first (bound flip)

    const int tid = threadIdx.x;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = d.m, n = d.n, ld = d.ld;
    const double eps = st->eps;
    if (st->iters >= st->max_iter) {   // pivots plus flips of this phase
        if (tid == 0) {
            st->status = LP_ITER_LIMIT;
            st->pivot_valid = 0;
        }
        return;
    }
    const double* drow = d.T + (size_t)m * ld;
    if (RULE == LP_PIVOT_BLAND) {
        if (tid < 64) {
            constexpr int K = 16;
            int e = INT_MAX;
            for (int base = 0; base < n && e == INT_MAX; base += 64 * K) {
                int first = INT_MAX;
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {   // (descending: the lane keeps its smallest hit)
                    const int j = base + k * 64 + tid;
                    if (j < n && d.nonbasic[j]) {
                        const double v = drow[j];
                        if (d.maximize ? (v > eps) : (v < -eps)) first = j;
                    }
                }
                e = lpdev::wave_min_i32(first);
            }
            if (tid == 0) s_enter = e == INT_MAX ? -1 : e;
        }
    } else {
        double* s_score = s_dyn + 2 * (d.m + 2) + 4;
        int* s_col = reinterpret_cast<int*>(s_score + 16);
        double best = -1.0;
        int col = INT_MAX;
        constexpr int K = 4;   // columns per thread and step: their loads are in flight together
        for (int j0 = tid; j0 < n; j0 += K * (int)blockDim.x) {
            double v[K], wj[K];
            bool nb[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int j = j0 + k * (int)blockDim.x;
                nb[k] = j < n && d.nonbasic[j] != 0;
                v[k] = j < n ? drow[j] : 0.0;
                wj[k] = j < n ? bd.w[j] : 1.0;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double s = (v[k] * v[k]) / wj[k];
                if (nb[k] && (d.maximize ? (v[k] > eps) : (v[k] < -eps)) && s > best) {
                    best = s;  // j ascending per thread: strict > keeps the smallest index
                    col = j0 + k * (int)blockDim.x;
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int oc = __shfl_xor(col, off, 64);
            if (ob > best || (ob == best && oc < col)) {
                best = ob;
                col = oc;
            }
        }
        if ((tid & 63) == 0) {
            s_score[tid >> 6] = best;
            s_col[tid >> 6] = col;
        }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < (int)(blockDim.x >> 6); ++q)
                if (s_score[q] > best || (s_score[q] == best && s_col[q] < col)) {
                    best = s_score[q];
                    col = s_col[q];
                }
            s_enter = col == INT_MAX ? -1 : col;
        }
    }
    __syncthreads();
    const int e = s_enter;
    if (e < 0) {
        if (tid == 0) {
            st->status = LP_OPTIMAL;
            st->pivot_valid = 0;
        }
        return;
    }
    // column e and the row values; a row that is no candidate holds NaN (Bland) or +inf (the chain of Devex)
    const double none = RULE == LP_PIVOT_BLAND ? NAN : INFINITY;
    for (int i = tid; i <= m; i += blockDim.x) {
        const double a = d.T[(size_t)i * ld + e];
        s_u[i] = a;
        if (i < m) {
            const double xb = d.T[(size_t)i * ld + n], u = bd.U[d.basis[i]];
            s_ratio[i] = (a > eps) ? xb / a : (a < -eps && u < INFINITY) ? (xb - u) / a : none;
        }
    }
    __syncthreads();
    const double ue = bd.U[e];
    if (tid < 64) {
        if (RULE == LP_PIVOT_BLAND) {
            double lmin = ue;
            for (int i = tid; i < m; i += 64) {
                const double v = s_ratio[i];
                if (v < lmin) lmin = v;
            }
            const double theta = lpdev::wave_ext_f64<false>(lmin);
            const double thr = theta + eps;
            int key = INT_MAX, pos = -1;
            if (tid == 0 && ue <= thr) {
                key = e;
                pos = -2;
            }
            for (int i = tid; i < m; i += 64)
                if (s_ratio[i] <= thr && d.basis[i] < key) {
                    key = d.basis[i];
                    pos = i;
                }
            const int kmin = lpdev::wave_min_i32(key);
            int r = -1;
            if (kmin != INT_MAX) r = __builtin_amdgcn_readlane(pos, (int)__builtin_ctzll(__ballot(key == kmin)));
            if (tid == 0) {
                s_leave = r;
                s_theta = theta;
            }
        } else {
            double theta;
            auto load = [&](int i, bool& ok) {
                ok = true;  // ineligible rows hold +inf, which the < scan never takes
                return s_ratio[i];
            };
            const int r = lpdev::wave_chain_select<false>(m, eps, theta, load);
            if (tid == 0) {
                s_leave = r;
                s_theta = theta;
            }
        }
    }
    __syncthreads();
    const int r = s_leave;
    bool flip;
    if (RULE == LP_PIVOT_BLAND) {
        if (!(s_theta < INFINITY) || r == -1) {   // (a finite theta* has a candidate at it: r == -1 cannot happen)
            if (tid == 0) {
                st->status = LP_UNBOUNDED;
                st->pivot_valid = 0;
            }
            return;
        }
        flip = r == -2;
    } else {
        if (r < 0 && !(ue < INFINITY)) {
            if (tid == 0) {
                st->status = LP_UNBOUNDED;
                st->pivot_valid = 0;
            }
            return;
        }
        flip = r < 0 || ue <= s_theta;
    }
    if (flip) {   // bound flip: e goes to its other bound, the basis (and every weight) stays
        for (int i = tid; i <= m; i += blockDim.x) {
            const size_t row = (size_t)i * ld;
            d.T[row + n] = fma(-ue, s_u[i], d.T[row + n]);
            d.T[row + e] = -s_u[i];
        }
        if (tid == 0) {
            bd.up[e] ^= 1;
            *bd.flips += 1;
            st->iters += 1;
            st->pivot_valid = 0;
        }
        return;
    }
    // pivot on row r; a_r < -eps: the leaving variable leaves at its upper bound and is complemented first
    const int old = d.basis[r];   // (every thread reads it, and Devex's old w_e, before the barrier below; thread 0
    const bool comp = s_u[r] < -eps;   //  writes basis[r] and w_old after it, and the loop writes neither weight)
    const double ur = comp ? -s_u[r] : s_u[r];
    const double we = RULE == LP_PIVOT_DEVEX ? bd.w[e] : 1.0;
    for (int i = tid; i <= m; i += blockDim.x)
        d.lcol[i] = (i == r) ? 1.0 / ur : -s_u[i] / ur;
    const double* trow = d.T + (size_t)r * ld;
    const double uold = bd.U[old];
    auto staged = [&](int j, double v) {
        if (comp) v = (j < n) ? -v : (j == n) ? uold - v : v;
        return (j == old) ? 1.0 : v;   // the leaving variable's own column: the unit column again
    };
    if (RULE == LP_PIVOT_DEVEX) {
        for (int j0 = tid; j0 < ld; j0 += 4 * (int)blockDim.x) {   // (four columns per step, as in the pricing)
            double a[4], wj[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + k * (int)blockDim.x;
                a[k] = j < ld ? trow[j] : 0.0;
                wj[k] = j < n ? bd.w[j] : 1.0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + k * (int)blockDim.x;
                if (j >= ld) continue;
                const double v = staged(j, a[k]);
                d.prow[j] = v;
                if (j < n && j != e && j != old) {
                    const double t = v / ur;
                    bd.w[j] = fmax(wj[k], (t * t) * we);
                }
            }
        }
    } else {
        for (int j = tid; j < ld; j += blockDim.x) d.prow[j] = staged(j, trow[j]);
    }
    __syncthreads();
    if (tid == 0) {
        if (RULE == LP_PIVOT_DEVEX) bd.w[old] = fmax(we / (ur * ur), 1.0);
        if (comp) bd.up[old] ^= 1;
        d.basis[r] = e;
        d.nonbasic[e] = 0;
        d.nonbasic[old] = 1;
        st->iters += 1;
        st->enter = e;
        st->leave = r;
        st->pivot_valid = 1;
    }
}

__global__ __launch_bounds__(1024) void k_simplex_select_bounded_bland(SimplexDev d, BoundedLargeDev bd) {
    select_bounded_rule<LP_PIVOT_BLAND>(d, bd);
}

__global__ __launch_bounds__(1024) void k_simplex_select_bounded_devex(SimplexDev d, BoundedLargeDev bd) {
    select_bounded_rule<LP_PIVOT_DEVEX>(d, bd);
}

// All d.n Devex weights back to exactly 1.0: queued at the start of every primal loop under LP_PIVOT_DEVEX
__global__ __launch_bounds__(256) void k_bounded_reset_weights(double* w, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) w[j] = 1.0;
}

// ---------------------------------------------------------------------------
// The bounded DUAL selector (step 6 of bounded_resolve_ref.c).  Both scans run on all 1024 threads through
// lpdev::block_chain_select, which replays the reference's sequential EPS-hysteresis chain exactly.
//   leaving:  v_t = xB_t if xB_t < -eps, else U_N(t) - xB_t if that is < -eps and U is finite, else ineligible;
//             r = the chain (min) over v_t in position order; none: optimal.  xB is read once, one row per thread,
//             into LDS; v_t goes to LDS too (the chain's near-tie replay reads it there);
//   complement: r violated above: row r is taken negated over the n columns with xB_r = U - xB_r, and up[N(r)]
//             toggles, whether or not an entering column is found;
//   entering: e = the chain (min) over d_j / a_j (max) or -d_j / a_j (min) of the non-basic j with a_j < -eps, a_j
//             the entry of the (complemented) row r, in index order; the quotients go to bd.q.  None: infeasible;
//   staging:  lcol, prow, basis, nonbasic, iters, enter, leave, pivot_valid as k_simplex_select_dual; prow is the
//             complemented row with the leaving variable's own entry +1 again.
// LDS: v[m+2] (then the entering column u[m+1]), xB[m], the chain scratch, 2 ints.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_simplex_select_dual_bounded(SimplexDev d, BoundedLargeDev bd) {
    SimplexState* st = d.state;
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_v = s_dyn;                     // m + 2: v_t, afterwards column e
    double* s_x = s_dyn + (d.m + 2);         // m (+ 2 of padding): xB
    lpdev::BlockChainScratch* sc = reinterpret_cast<lpdev::BlockChainScratch*>(s_dyn + 2 * (d.m + 2));

    const int tid = threadIdx.x;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = d.m, n = d.n, ld = d.ld;
    const double eps = st->eps;
    if (st->iters >= st->max_iter) {
        if (tid == 0) {
            st->status = LP_ITER_LIMIT;
            st->pivot_valid = 0;
        }
        return;
    }
    // leaving position
    double best;
    auto violation = [&](int t) {
        const double xb = d.T[(size_t)t * ld + n], u = bd.U[d.basis[t]];
        s_x[t] = xb;
        return (xb < -eps) ? xb : (u < INFINITY && u - xb < -eps) ? u - xb : INFINITY;
    };
    const int r = lpdev::block_chain_select<false, true>(m, eps, best, violation, s_v, sc);
    if (r < 0) {
        if (tid == 0) {
            st->status = LP_OPTIMAL;
            st->pivot_valid = 0;
        }
        return;
    }
    // (every thread reads basis[r] and nonbasic[] before the barriers below; thread 0 writes them after the last)
    const int old = d.basis[r];
    const bool comp = !(s_x[r] < -eps);   // violated above: the complement of N(r) is what is below 0
    const double uold = bd.U[old];
    // entering column
    const double* trow = d.T + (size_t)r * ld;
    const double* drow = d.T + (size_t)m * ld;
    const bool maxi = d.maximize != 0;
    auto quotient = [&](int j) {
        const double t = trow[j], a = comp ? -t : t;
        if (!(d.nonbasic[j] != 0 && a < -eps)) return (double)INFINITY;
        return maxi ? drow[j] / a : -drow[j] / a;
    };
    const int e = lpdev::block_chain_select<false, true>(n, eps, best, quotient, bd.q, sc);
    if (e < 0) {   // row r sums non-negative terms to a negative right-hand side
        if (tid == 0) {
            if (comp) bd.up[old] ^= 1;
            st->status = LP_INFEASIBLE;
            st->pivot_valid = 0;
        }
        return;
    }
    // stage the pivot on (r, e); column e of the complemented row r changes sign with it
    for (int i = tid; i <= m; i += blockDim.x) s_v[i] = d.T[(size_t)i * ld + e];
    __syncthreads();
    const double ur = comp ? -s_v[r] : s_v[r];
    for (int i = tid; i <= m; i += blockDim.x)
        d.lcol[i] = (i == r) ? 1.0 / ur : -s_v[i] / ur;
    for (int j = tid; j < ld; j += blockDim.x) {
        double v = trow[j];
        if (comp) v = (j < n) ? -v : (j == n) ? uold - v : v;
        if (j == old) v = 1.0;   // the leaving variable's own column: the unit column again (a no-op without comp)
        d.prow[j] = v;
    }
    __syncthreads();
    if (tid == 0) {
        if (comp) bd.up[old] ^= 1;
        d.basis[r] = e;
        d.nonbasic[e] = 0;
        d.nonbasic[old] = 1;
        const int it = st->iters;
        if (it < d.trace_cap) {
            d.trace_enter[it] = e;
            d.trace_leave[it] = r;
        }
        st->iters = it + 1;
        st->enter = e;
        st->leave = r;
        st->pivot_valid = 1;
    }
}

// ---------------------------------------------------------------------------
// The bounded dual selector under Devex pricing (LP_DUAL_DEVEX; tests/ref/bounded_resolve_dual_rules_ref.c is the
// definition).  Everything but the leaving choice and the weights is k_simplex_select_dual_bounded's: the complement,
// the entering chain with its quotients in bd.q, the staging of lcol / prow, the trace.
//   weights:  bd.w[0 .. m), one per basis position, all exactly 1.0 when the dual loop starts (the host resets them
//             on the stream);
//   leaving:  the arg-max of (v_t * v_t) / w_t over the violated positions by the whole workgroup: each thread strides
//             over its positions (m may exceed the 1024 threads) with a strict >, the waves and then the workgroup
//             combine on (score, position) with exact ties to the smaller position, as k_simplex_select_bounded_devex
//             does for its columns.  A NaN score fails every comparison and is never taken.  Every thread combines the
//             sixteen published wave results itself, so all of them hold the same r without another barrier;
//   update:   in the loop that stages lcol, from column e in LDS, a = T[r][e] as the complement left it and the old
//             w_r (read by every thread right after the selection, several barriers ahead of its rewrite):
//             w_i = cand if cand = (g * g) * w_r > w_i, g = T[i][e] / a, for i != r; w_r = max(w_r / (a * a), 1.0) by
//             the thread that owns r.  An infeasible exit updates nothing.  No multiply feeds an add.
// LDS: k_simplex_select_dual_bounded's plus the sixteen wave results (16 doubles + 16 ints):
// 16 (m + 2) + 208 + 192 bytes <= 156 KiB, m <= 9957.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_simplex_select_dual_bounded_devex(SimplexDev d, BoundedLargeDev bd) {
    SimplexState* st = d.state;
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_v = s_dyn;                     // m + 2: column e
    double* s_x = s_dyn + (d.m + 2);         // m (+ 2 of padding): xB
    lpdev::BlockChainScratch* sc = reinterpret_cast<lpdev::BlockChainScratch*>(s_dyn + 2 * (d.m + 2));
    double* s_score = reinterpret_cast<double*>(sc + 1);   // the sixteen wave results of the leaving choice
    int* s_pos = reinterpret_cast<int*>(s_score + 16);

    const int tid = threadIdx.x;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = d.m, n = d.n, ld = d.ld;
    const double eps = st->eps;
    if (st->iters >= st->max_iter) {
        if (tid == 0) {
            st->status = LP_ITER_LIMIT;
            st->pivot_valid = 0;
        }
        return;
    }
    // leaving position
    double best = -1.0;
    int r = INT_MAX;
    for (int t = tid; t < m; t += blockDim.x) {
        const double xb = d.T[(size_t)t * ld + n], u = bd.U[d.basis[t]], wt = bd.w[t];
        s_x[t] = xb;
        const double v = (xb < -eps) ? xb : u - xb;
        const double s = (v * v) / wt;
        if ((xb < -eps || (u < INFINITY && v < -eps)) && s > best) {
            best = s;   // t ascending per thread: strict > keeps the smallest position
            r = t;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int op = __shfl_xor(r, off, 64);
        if (ob > best || (ob == best && op < r)) {
            best = ob;
            r = op;
        }
    }
    if ((tid & 63) == 0) {
        s_score[tid >> 6] = best;
        s_pos[tid >> 6] = r;
    }
    __syncthreads();
    best = s_score[0];
    r = s_pos[0];
    for (int q = 1; q < (int)(blockDim.x >> 6); ++q)
        if (s_score[q] > best || (s_score[q] == best && s_pos[q] < r)) {
            best = s_score[q];
            r = s_pos[q];
        }
    if (r == INT_MAX) {
        if (tid == 0) {
            st->status = LP_OPTIMAL;
            st->pivot_valid = 0;
        }
        return;
    }
    // (every thread reads basis[r], w[r] and nonbasic[] before the barriers below; they are written after the last)
    const int old = d.basis[r];
    const double wr = bd.w[r];
    const bool comp = !(s_x[r] < -eps);   // violated above: the complement of N(r) is what is below 0
    const double uold = bd.U[old];
    // entering column
    const double* trow = d.T + (size_t)r * ld;
    const double* drow = d.T + (size_t)m * ld;
    const bool maxi = d.maximize != 0;
    auto quotient = [&](int j) {
        const double t = trow[j], a = comp ? -t : t;
        if (!(d.nonbasic[j] != 0 && a < -eps)) return (double)INFINITY;
        return maxi ? drow[j] / a : -drow[j] / a;
    };
    const int e = lpdev::block_chain_select<false, true>(n, eps, best, quotient, bd.q, sc);
    if (e < 0) {   // row r sums non-negative terms to a negative right-hand side
        if (tid == 0) {
            if (comp) bd.up[old] ^= 1;
            st->status = LP_INFEASIBLE;
            st->pivot_valid = 0;
        }
        return;
    }
    // stage the pivot on (r, e); column e of the complemented row r changes sign with it
    for (int i = tid; i <= m; i += blockDim.x) s_v[i] = d.T[(size_t)i * ld + e];
    __syncthreads();
    const double ur = comp ? -s_v[r] : s_v[r];
    for (int i = tid; i <= m; i += blockDim.x) {
        d.lcol[i] = (i == r) ? 1.0 / ur : -s_v[i] / ur;
        if (i == r) {
            bd.w[i] = fmax(wr / (ur * ur), 1.0);
        } else if (i < m) {
            const double g = s_v[i] / ur;
            const double cand = (g * g) * wr;
            if (cand > bd.w[i]) bd.w[i] = cand;
        }
    }
    for (int j = tid; j < ld; j += blockDim.x) {
        double v = trow[j];
        if (comp) v = (j < n) ? -v : (j == n) ? uold - v : v;
        if (j == old) v = 1.0;   // the leaving variable's own column: the unit column again (a no-op without comp)
        d.prow[j] = v;
    }
    __syncthreads();
    if (tid == 0) {
        if (comp) bd.up[old] ^= 1;
        d.basis[r] = e;
        d.nonbasic[e] = 0;
        d.nonbasic[old] = 1;
        const int it = st->iters;
        if (it < d.trace_cap) {
            d.trace_enter[it] = e;
            d.trace_leave[it] = r;
        }
        st->iters = it + 1;
        st->enter = e;
        st->leave = r;
        st->pivot_valid = 1;
    }
}

// ---------------------------------------------------------------------------
// The two bounded dual selectors with the bound-flipping ratio test (LP_DUAL_RATIO_LONG_STEP;
// tests/ref/bounded_resolve_long_step_ref.c is the definition).  DEVEX = false: the leaving choice of
// k_simplex_select_dual_bounded; true: that of k_simplex_select_dual_bounded_devex with its weight update.  The
// complement, the first entering chain with its quotients in bd.q, the staging and the trace are theirs.
//   round:    column e goes to LDS (it is staged from there if the round ends in the pivot).  With a the entry of the
//             complemented row r and xbr its right-hand side, both as this launch has left them, e is flipped when
//             U_e is finite and fma(-U_e, a, xbr) < -eps: row r stays violated with e at its other bound;
//   flip:     the primal selector's, by the whole workgroup, rows 0 .. m (strided beyond 1024, the cost row included):
//             T[i][n] = fma(-U_e, T[i][e], T[i][n]), T[i][e] negated; up[e] toggles and bd.flips counts it.  Row r's
//             complement is virtual here, so its entry of column e is flipped as the complemented view sees it
//             (a = -T[r][e]; the stored T[r][e] is negated like every other row's) and its right-hand side lives in
//             xbr alone, which every thread carries through the same operations and which is staged as prow[n]; the
//             stored T[r][n] of a complemented row is left as it was, for k_simplex_update writes row r from prow;
//   rescan:   q[e] = +inf, a barrier, and block_chain_select again over bd.q as it stands: the flipped column has
//             a > eps now and nothing else of row r or of the cost row has changed, so this is the reference's rescan.
//             None left: infeasible, with the flips made and the complement's flag kept.
// st->iters counts the dual pivots only, as max_iter bounds them; a launch makes at most n flips.
// LDS: that of the selector it extends; no more.
// ---------------------------------------------------------------------------
// The two pieces of k_simplex_select_dual_bounded_long that restate the textbook selectors, which themselves stay as
// they are.  Every thread of the 1024-thread workgroup calls them.
// The leaving choice of k_simplex_select_dual_bounded_devex: xB goes to s_x, the result is the same in every thread
// (-1: no position violated).
__device__ __forceinline__ int dual_devex_leaving(const SimplexDev& d, const BoundedLargeDev& bd, double eps, double* s_x,
                                                  double* s_score, int* s_pos) {
    const int tid = threadIdx.x, m = d.m, n = d.n, ld = d.ld;
    double best = -1.0;
    int r = INT_MAX;
    for (int t = tid; t < m; t += blockDim.x) {
        const double xb = d.T[(size_t)t * ld + n], u = bd.U[d.basis[t]], wt = bd.w[t];
        s_x[t] = xb;
        const double v = (xb < -eps) ? xb : u - xb;
        const double s = (v * v) / wt;
        if ((xb < -eps || (u < INFINITY && v < -eps)) && s > best) {
            best = s;   // t ascending per thread: strict > keeps the smallest position
            r = t;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int op = __shfl_xor(r, off, 64);
        if (ob > best || (ob == best && op < r)) {
            best = ob;
            r = op;
        }
    }
    if ((tid & 63) == 0) {
        s_score[tid >> 6] = best;
        s_pos[tid >> 6] = r;
    }
    __syncthreads();
    best = s_score[0];
    r = s_pos[0];
    for (int q = 1; q < (int)(blockDim.x >> 6); ++q)
        if (s_score[q] > best || (s_score[q] == best && s_pos[q] < r)) {
            best = s_score[q];
            r = s_pos[q];
        }
    return r == INT_MAX ? -1 : r;
}

// The staging of the pivot on (r, e) for k_simplex_update, as the textbook selectors do it, from column e in s_v:
// ur is the entry of the (complemented) row r in column e and xbr that row's right-hand side, which goes to prow[n]
// as carried, not as stored.
__device__ __forceinline__ void dual_long_stage(const SimplexDev& d, const BoundedLargeDev& bd, int r, int e, int old,
                                                bool comp, double ur, double xbr, const double* s_v) {
    SimplexState* st = d.state;
    const int tid = threadIdx.x, m = d.m, n = d.n, ld = d.ld;
    const double* trow = d.T + (size_t)r * ld;
    for (int i = tid; i <= m; i += blockDim.x) d.lcol[i] = (i == r) ? 1.0 / ur : -s_v[i] / ur;
    for (int j = tid; j < ld; j += blockDim.x) {
        double v = trow[j];
        if (comp) v = (j < n) ? -v : v;
        if (j == n) v = xbr;
        if (j == old) v = 1.0;   // the leaving variable's own column: the unit column again (a no-op without comp)
        d.prow[j] = v;
    }
    __syncthreads();
    if (tid == 0) {
        if (comp) bd.up[old] ^= 1;
        d.basis[r] = e;
        d.nonbasic[e] = 0;
        d.nonbasic[old] = 1;
        const int it = st->iters;
        if (it < d.trace_cap) {
            d.trace_enter[it] = e;
            d.trace_leave[it] = r;
        }
        st->iters = it + 1;
        st->enter = e;
        st->leave = r;
        st->pivot_valid = 1;
    }
}

template <bool DEVEX>
__global__ __launch_bounds__(1024) void k_simplex_select_dual_bounded_long(SimplexDev d, BoundedLargeDev bd) {
    SimplexState* st = d.state;
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_v = s_dyn;                     // m + 2: v_t (Dantzig), afterwards column e
    double* s_x = s_dyn + (d.m + 2);         // m (+ 2 of padding): xB
    lpdev::BlockChainScratch* sc = reinterpret_cast<lpdev::BlockChainScratch*>(s_dyn + 2 * (d.m + 2));
    double* s_score = reinterpret_cast<double*>(sc + 1);   // DEVEX: the sixteen wave results of the leaving choice
    int* s_pos = reinterpret_cast<int*>(s_score + 16);

    const int tid = threadIdx.x;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = d.m, n = d.n, ld = d.ld;
    const double eps = st->eps;
    if (st->iters >= st->max_iter) {
        if (tid == 0) {
            st->status = LP_ITER_LIMIT;
            st->pivot_valid = 0;
        }
        return;
    }
    // leaving position
    double best;
    int r;
    if constexpr (DEVEX) {
        r = dual_devex_leaving(d, bd, eps, s_x, s_score, s_pos);
    } else {
        auto violation = [&](int t) {
            const double xb = d.T[(size_t)t * ld + n], u = bd.U[d.basis[t]];
            s_x[t] = xb;
            return (xb < -eps) ? xb : (u < INFINITY && u - xb < -eps) ? u - xb : INFINITY;
        };
        r = lpdev::block_chain_select<false, true>(m, eps, best, violation, s_v, sc);
    }
    if (r < 0) {
        if (tid == 0) {
            st->status = LP_OPTIMAL;
            st->pivot_valid = 0;
        }
        return;
    }
    // (every thread reads basis[r], w[r] and nonbasic[] before the barriers below; they are written after the last)
    const int old = d.basis[r];
    const double wr = DEVEX ? bd.w[r] : 0.0;
    const bool comp = !(s_x[r] < -eps);   // violated above: the complement of N(r) is what is below 0
    const double uold = bd.U[old];
    double xbr = comp ? uold - s_x[r] : s_x[r];   // the complemented row's right-hand side, the same in every thread
    // entering column
    const double* trow = d.T + (size_t)r * ld;
    const double* drow = d.T + (size_t)m * ld;
    const bool maxi = d.maximize != 0;
    auto quotient = [&](int j) {
        const double t = trow[j], a = comp ? -t : t;
        if (!(d.nonbasic[j] != 0 && a < -eps)) return (double)INFINITY;
        return maxi ? drow[j] / a : -drow[j] / a;
    };
    int e = lpdev::block_chain_select<false, true>(n, eps, best, quotient, bd.q, sc);
    double ur;
    for (;;) {
        if (e < 0) {   // row r sums non-negative terms to a negative right-hand side, at either bound of every column
            if (tid == 0) {
                if (comp) bd.up[old] ^= 1;
                st->status = LP_INFEASIBLE;
                st->pivot_valid = 0;
            }
            return;
        }
        // column e; the entry of the complemented row r changes sign with it
        for (int i = tid; i <= m; i += blockDim.x) s_v[i] = d.T[(size_t)i * ld + e];
        __syncthreads();
        ur = comp ? -s_v[r] : s_v[r];
        const double ue = bd.U[e];
        if (!(ue < INFINITY && fma(-ue, ur, xbr) < -eps)) break;
        // bound flip: row r stays violated with e at its other bound
        for (int i = tid; i <= m; i += blockDim.x) {
            const size_t row = (size_t)i * ld;
            if (i != r || !comp) d.T[row + n] = fma(-ue, s_v[i], d.T[row + n]);
            d.T[row + e] = -s_v[i];
        }
        xbr = fma(-ue, ur, xbr);
        if (tid == 0) {
            bd.up[e] ^= 1;
            *bd.flips += 1;
            bd.q[e] = INFINITY;
        }
        __syncthreads();   // q[e], and every read of s_v, ahead of the next round
        e = lpdev::block_chain_select<false, false>(n, eps, best, [&](int j) { return bd.q[j]; }, bd.q, sc);
    }
    // stage the pivot on (r, e); under Devex the weights move with it
    if constexpr (DEVEX) {
        for (int i = tid; i < m; i += blockDim.x) {
            if (i == r) {
                bd.w[i] = fmax(wr / (ur * ur), 1.0);
            } else {
                const double g = s_v[i] / ur;
                const double cand = (g * g) * wr;
                if (cand > bd.w[i]) bd.w[i] = cand;
            }
        }
    }
    dual_long_stage(d, bd, r, e, old, comp, ur, xbr, s_v);
}

// Which loop lp_simplex_bounded_resolve_large runs: the bounded form of k_simplex_classify.  st->pad0 = bit 0 some
// basis position violated (xB_t < -eps, or U_N(t) finite and U_N(t) - xB_t < -eps), bit 1 dual infeasible (some
// non-basic d_j > eps for max, d_j < -eps for min).  One workgroup.
__global__ __launch_bounds__(1024) void k_simplex_classify_bounded(SimplexDev d, BoundedLargeDev bd, double eps) {
    const int tid = threadIdx.x, m = d.m, n = d.n, ld = d.ld;
    int pinf = 0, dinf = 0;
    for (int t = tid; t < m; t += blockDim.x) {
        const double xb = d.T[(size_t)t * ld + n], u = bd.U[d.basis[t]];
        if (xb < -eps || (u < INFINITY && u - xb < -eps)) pinf = 1;
    }
    const double* drow = d.T + (size_t)m * ld;
    for (int j = tid; j < n; j += blockDim.x)
        if (d.nonbasic[j] && (d.maximize ? (drow[j] > eps) : (drow[j] < -eps))) dinf = 1;
    pinf = __syncthreads_or(pinf);
    dinf = __syncthreads_or(dinf);
    if (tid == 0) d.state->pad0 = (pinf ? 1 : 0) | (dinf ? 2 : 0);
}

// (LP_DUAL_DEVEX: the sixteen wave results of the leaving choice, 16 doubles + 16 ints, behind the chain scratch)
size_t select_dual_bounded_lds_bytes(const lp_simplex_problem* p, int dual_rule = LP_DUAL_DANTZIG) {
    return sizeof(double) * 2 * (size_t)(p->dev.m + 2) + sizeof(lpdev::BlockChainScratch) +
           (dual_rule == LP_DUAL_DEVEX ? 16 * 8 + 16 * 4 : 0);
}

// (Devex: the sixteen wave results of the pricing, 16 doubles + 16 ints, behind the two ints)
size_t select_bounded_lds_bytes(const lp_simplex_problem* p, int rule) {
    return sizeof(double) * (2 * (size_t)(p->dev.m + 2) + 2) + 16 + (rule == LP_PIVOT_DEVEX ? 16 * 8 + 16 * 4 : 0);
}

using BoundedSelector = void (*)(SimplexDev, BoundedLargeDev);
BoundedSelector bounded_selector(int rule) {
    return rule == LP_PIVOT_BLAND   ? k_simplex_select_bounded_bland
           : rule == LP_PIVOT_DEVEX ? k_simplex_select_bounded_devex
                                    : k_simplex_select_bounded;
}

// (the long-step forms need the LDS of the selector they extend: select_dual_bounded_lds_bytes by dual_rule)
BoundedSelector bounded_dual_selector(int dual_rule, int dual_ratio) {
    if (dual_ratio == LP_DUAL_RATIO_LONG_STEP)
        return dual_rule == LP_DUAL_DEVEX ? k_simplex_select_dual_bounded_long<true> : k_simplex_select_dual_bounded_long<false>;
    return dual_rule == LP_DUAL_DEVEX ? k_simplex_select_dual_bounded_devex : k_simplex_select_dual_bounded;
}

}  // namespace

int lp_bounded_large_prepare(lp_simplex_problem* p, int rule) {
    const size_t shm = select_bounded_lds_bytes(p, rule);
    if (shm > 156 * 1024) LP_FAIL(p->ctx, LP_BAD_ARG, "lp_simplex_bounded_large: m too large for the selector's LDS");
    LP_HIP(p->ctx, lp_lds_opt_in(reinterpret_cast<const void*>(bounded_selector(rule)), shm));
    return LP_OPTIMAL;
}

void lp_bounded_large_reset_weights(lp_simplex_problem* p, const BoundedLargeDev& bd, bool dual) {
    const int n = dual ? p->dev.m : p->dev.n;
    hipLaunchKernelGGL(k_bounded_reset_weights, (n + 255) / 256, 256, 0, p->ctx->stream, bd.w, n);
}

int lp_bounded_large_queue(lp_simplex_problem* p, const BoundedLargeDev& bd, int batch, int rule, bool dual,
                           int dual_rule, int dual_ratio) {
    const size_t shm = dual ? select_dual_bounded_lds_bytes(p, dual_rule) : select_bounded_lds_bytes(p, rule);
    const BoundedSelector select = dual ? bounded_dual_selector(dual_rule, dual_ratio) : bounded_selector(rule);
    for (int k = 0; k < batch; ++k) {
        hipLaunchKernelGGL(select, 1, 1024, shm, p->ctx->stream, p->dev, bd);
        lp_simplex_launch_update(p);
    }
    return 2 * batch;
}

int lp_bounded_large_classify(lp_simplex_problem* p, const BoundedLargeDev& bd, double eps, int* flags) {
    lp_context* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_simplex_classify_bounded, 1, 1024, 0, s, p->dev, bd, eps);
    LP_HIP(ctx, hipMemcpyAsync(p->h_state, p->dev.state, sizeof(SimplexState), hipMemcpyDeviceToHost, s));
    LP_HIP(ctx, hipStreamSynchronize(s));
    LP_HIP(ctx, hipGetLastError());
    *flags = p->h_state->pad0;
    return LP_OPTIMAL;
}

int lp_bounded_dual_prepare(lp_simplex_problem* p, int dual_rule, int dual_ratio) {
    const size_t shm = select_dual_bounded_lds_bytes(p, dual_rule);
    if (shm > 156 * 1024)
        LP_FAIL(p->ctx, LP_BAD_ARG, "lp_simplex_bounded_resolve_large: m too large for the dual selector's LDS");
    LP_HIP(p->ctx, lp_lds_opt_in(reinterpret_cast<const void*>(bounded_dual_selector(dual_rule, dual_ratio)), shm));
    return LP_OPTIMAL;
}
