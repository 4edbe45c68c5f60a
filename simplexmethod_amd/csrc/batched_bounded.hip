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
//
// FITS (lp_simplex_bounded_fits): lp_bounded_lds_bytes(m, n) <= 160 KB, one CU's LDS.  Canonical 64 x 192 takes 105 KB.
// There is no host fallback: larger shapes get LP_BAD_ARG.
#include <climits>

#include "device_select.hpp"
#include "lp_internal.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"
#include "batched_bounded_carve.hpp"

namespace {

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_bounded(BatchedBoundedDev d) {
    constexpr bool BLAND = false;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    char* base = reinterpret_cast<char*>(smem);
    const int m = d.m, n = d.n, W = n + 1;
    const BoundedCarve K = bounded_carve(m, n);
    const int pitch = K.pitch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = reinterpret_cast<double*>(base + K.T);
    double* prow = reinterpret_cast<double*>(base + K.prow);
    double* lcol = reinterpret_cast<double*>(base + K.lcol);
    double* U = reinterpret_cast<double*>(base + K.U);
    double* lov = reinterpret_cast<double*>(base + K.lov);
    int* slotvar = reinterpret_cast<int*>(base + K.slotvar);
    int* basis = reinterpret_cast<int*>(base + K.basis);
    int* up = reinterpret_cast<int*>(base + K.up);
    int* pub = pubs->v;   // [0] entering slot, [1] leaving position, [2] action / infeasible, [3] hi < lo

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* lo = d.lo + (size_t)lp * n;
    const double* hi = d.hi + (size_t)lp * n;
    const double eps = d.eps;

    // ---- load: slots = original columns in order, basis = the artificials by position, nothing complemented
    for (int s = tid; s < n; s += NT) {
        const double l = lo[s];
        slotvar[s] = s;
        up[s] = 0;
        lov[s] = l;
        U[s] = hi[s] - l;
    }
    for (int t = tid; t < m; t += NT) basis[t] = n + t;
    for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
        const int s = e / m, i = e - s * m;
        T[(size_t)i * pitch + s] = A[e];
    }
    __syncthreads();
    // ---- shift (one chain per row, lo_j == 0 skipped) and the auxiliary problem's sign changes
    for (int i = tid; i < m; i += NT) {
        double acc = b[i];
        for (int j = 0; j < n; ++j) {
            const double l = lov[j];
            if (l != 0.0) acc = fma(-T[(size_t)i * pitch + j], l, acc);
        }
        const bool flip = acc < -eps;
        T[(size_t)i * pitch + n] = flip ? -acc : acc;
        lcol[i] = flip ? -1.0 : 1.0;
    }
    if (wave == 0) {
        int bad = 0;
        for (int s = lane; s < n; s += 64)
            if (U[s] < 0.0) bad = 1;
        bad = __any(bad);
        if (lane == 0) pub[3] = bad;
    }
    __syncthreads();
    const bool crossed = pub[3] != 0;
    if (!crossed) {
        for (int e = tid; e < m * n; e += NT) {
            const int i = e / n, s = e - i * n;
            if (lcol[i] < 0.0) T[(size_t)i * pitch + s] = -T[(size_t)i * pitch + s];
        }
        __syncthreads();
        // ---- phase-I reduced costs: the artificial basis' crash, one serial chain per column
        for (int j = tid; j < W; j += NT) {
            double dj = 0.0;
            for (int t = 0; t < m; ++t) dj = fma(-1.0, T[(size_t)t * pitch + j], dj);
            T[(size_t)m * pitch + j] = dj;
        }
        __syncthreads();
    }

#include "batched_lds_loop.hpp"
#include "batched_bounded_loop.hpp"
    (void)simplex;   // (batched_lds_loop.hpp's unbounded loop: only its pivot is used here)

    int it[4] = {0, 0, 0, 0};
    int status = LP_INFEASIBLE;
    if (!crossed) {
        // ---- phase I: minimise the sum of the artificials; every slot may enter
        status = bounded_simplex(false, false, it[0], it[3]);
        __syncthreads();
        if (status == LP_OPTIMAL) {
            // the artificials' values by artificial index, summed in that order
            for (int i = tid; i < m; i += NT) lcol[i] = 0.0;
            __syncthreads();
            for (int t = tid; t < m; t += NT)
                if (basis[t] >= n) lcol[basis[t] - n] = T[(size_t)t * pitch + n];
            __syncthreads();
            if (tid == 0) {
                double sum = 0.0;
                for (int i = 0; i < m; ++i) sum += lcol[i];
                pub[2] = sum > eps;
            }
            __syncthreads();
            if (pub[2]) status = LP_INFEASIBLE;
        }
        // ---- drive-out: every position still holding an artificial, in ascending order
        for (int pos = 0; pos < m && status == LP_OPTIMAL; ++pos) {
            if (basis[pos] < n) continue;
            if (wave == 0) {   // the eligible slot of smallest variable index
                int kbest = INT_MAX, sbest = -1;
                for (int s = lane; s < n; s += 64) {
                    const int k = slotvar[s];
                    if (k < n && k < kbest && fabs(T[(size_t)pos * pitch + s]) > eps) {
                        kbest = k;
                        sbest = s;
                    }
                }
                const int kmin = (int)lpdev::wave_ext_u32<false>((unsigned)kbest);
                const int s0 =
                    kmin == INT_MAX ? -1 : __builtin_amdgcn_readlane(sbest, (int)__builtin_ctzll(__ballot(kbest == kmin)));
                if (lane == 0) pub[0] = s0;
            }
            __syncthreads();
            const int s = pub[0];
            if (s < 0) {
                status = LP_SINGULAR;
                break;
            }
            pivot(pos, s);
            ++it[1];
        }
        __syncthreads();
        if (status == LP_OPTIMAL) {
            // ---- phase-II reduced costs: c' (c_j, or -c_j for a complemented column) priced out over the basis in
            // position order
            auto cost = [&](int k) -> double { return k < n ? (up[k] ? -c[k] : c[k]) : 0.0; };
            for (int t = tid; t < m; t += NT) lcol[t] = -cost(basis[t]) / 1.0;
            __syncthreads();
            for (int j = tid; j < W; j += NT) {
                double dj = j < n ? cost(slotvar[j]) : 0.0;
                for (int t = 0; t < m; ++t) dj = fma(lcol[t], T[(size_t)t * pitch + j], dj);
                T[(size_t)m * pitch + j] = dj;
            }
            __syncthreads();
            // ---- phase II: artificial slots never enter; max_iter counts from 0 again
            status = bounded_simplex(true, d.maximize != 0, it[2], it[3]);
            __syncthreads();
        }
    }
    // ---- outputs: x_j = lo_j + (up_j ? U_j - v_j : v_j) (lo_j == 0: no addition) for LP_OPTIMAL; basis, flags and
    // counters always (an LP with hi < lo: the starting basis, nothing complemented, zero counters)
    if (status == LP_OPTIMAL) {
        for (int j = tid; j < n; j += NT) prow[j] = 0.0;
        __syncthreads();
        for (int t = tid; t < m; t += NT)
            if (basis[t] < n) prow[basis[t]] = T[(size_t)t * pitch + n];
        __syncthreads();
        double* x = d.x + (size_t)lp * n;
        for (int j = tid; j < n; j += NT) {
            const double v = prow[j];
            const double w = up[j] ? U[j] - v : v;
            x[j] = lov[j] == 0.0 ? w : lov[j] + w;
        }
    }
    for (int t = tid; t < m; t += NT) d.basis_out[(size_t)lp * m + t] = basis[t];
    for (int j = tid; j < n; j += NT) d.at_upper[(size_t)lp * n + j] = up[j];
    if (tid == 0) {
        int* io = d.iters + (size_t)lp * 4;
        io[0] = it[0];
        io[1] = it[1];
        io[2] = it[2];
        io[3] = it[3];
        d.status[lp] = status;
    }
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

int lp_batched_bounded_launch(lp_context* ctx, const BatchedBoundedDev& d) {
    if (!lp_bounded_fits_shape(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "batched bounded simplex: the shape does not fit one CU's LDS");
    return lp_launch_per_lp(ctx, (size_t)(d.m + 1) * (d.n + 1), k_batched_bounded<256>, k_batched_bounded<1024>,
                            lp_bounded_lds_bytes(d.m, d.n, nullptr), d);
}
