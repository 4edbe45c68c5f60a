// basis_parametric_cost.hip — the parametric cost path z*(t) = opt { (c + t g).x : A x = b, x >= 0 } from a given
// optimal basis, for t from 0 up to t_max, exactly as tests/ref/parametric_cost_ref.c states it:
//   - install the basis: the re-solve's crash on [A | b; c | 0; g | 0] (batched_resolve_crash.hpp) over all m+2 rows,
//     so d (row m) and delta (row m+1) are the reduced costs of c and of g;
//   - start check: no xB_t < -eps and no non-basic d_j > eps (max) / d_j < -eps (min), else LP_BAD_ARG;
//   - per segment k (from t_k): obj = the chain fma(fma(t_k, g_B, c_B), xB, s) and slope = the chain
//     fma(g_B, xB, s) in position order, on one lane; the breakpoint is the first strict minimum of
//     tau_j = -d_j / delta_j over the non-basic j with delta_j > eps (max) / delta_j < -eps (min) (basis_crash.hpp's
//     take), t* = max(tau, t_k); then the primal ratio test over the entering column (the re-solve's primal loop),
//     and one pivot.  The path ends at t_max (LP_OPTIMAL), at t* with no leaving row (LP_UNBOUNDED) or at t* after
//     max_breaks pivots (LP_ITER_LIMIT).
//
// k_batched_parametric_cost<NT, MX>: one LP per workgroup, the (m+2) x pitch tableau in LDS in batched_resolve.hip's
// layout (b in slot n).  batched_lds_loop.hpp's pivot stops at row m, so the kernel has its own over m+2 rows, which
// batched_resolve_crash.hpp (included unchanged) calls.  The sense is a template parameter.
//
// Shapes beyond lp_basis_parametric_cost_fits: the single-LP launch pair updates rows 0..m only, and a non-pivot
// row's new value depends only on itself and the pivot row.  So lp_simplex_crash runs twice on the (m+2)-row tableau:
// first with g in row m (its result is copied to row m+1), then with c in row m; the A and b rows come out the same
// both times.  Then k_pc_begin checks the start, and k_pc_select<MX> (one workgroup: the segment record, the tau
// reduction, the ratio test of device_select.hpp, the pivot staged over m+2 rows) and the existing k_simplex_update
// on a view of m+1 constraint rows run once per breakpoint, queued in batches under the polling loop.
#include <cfloat>

#include "basis_crash.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"
#include "device_select.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kRunning = -100;   // SimplexState::status while pivoting
enum { kGoOn = 0, kEndTMax = 1, kEndUnbounded = 2, kEndLimit = 3 };

__host__ __device__ inline int parametric_cost_status(int code) {
    return code == kEndUnbounded ? LP_UNBOUNDED : code == kEndLimit ? LP_ITER_LIMIT : LP_OPTIMAL;
}

template <int NT, bool MX>
__global__ __launch_bounds__(NT) void k_batched_parametric_cost(BasisParametricDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int m = d.m, n = d.n, W = n + 1, pitch = d.pitch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve (batched_resolve.hip's, two cost rows)
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = smem + sizeof(Published) / 8;             // (m+2) x pitch
    double* prow = T + (size_t)(m + 2) * pitch;           // W
    double* lcol = prow + W;                              // m+2
    int* slotvar = reinterpret_cast<int*>(lcol + m + 2);  // n
    int* basis = slotvar + n;                             // m
    int* pub = pubs->v;   // [0] entering slot / crash row, [1] leaving position, [2] verdict / end code, [3] block_any

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* g = d.dir + (size_t)lp * n;
    const int* N = d.basis + (size_t)lp * m;
    const double eps = d.eps;
    const int MB = d.max_breaks;
    double* t_out = d.t + (size_t)lp * (MB + 2);
    double* obj_out = d.obj + (size_t)lp * (MB + 2);
    double* slope_out = d.slope + (size_t)lp * (MB + 1);
    int* enter_out = d.enter + (size_t)lp * (MB + 1);
    int* leave_out = d.leave + (size_t)lp * (MB + 1);
    constexpr int ANY_WORD = 3;   // block_any's word of pub
#include "batched_block_any.hpp"
    // sum_t fma(tt, g[basis[t]], c[basis[t]]) * xB_t, the chain in position order (one lane)
    auto value_at = [&](double tt) {
        double s = 0.0;
        for (int t = 0; t < m; ++t) s = fma(fma(tt, g[basis[t]], c[basis[t]]), T[(size_t)t * pitch + n], s);
        return s;
    };

    const int run = d.run_status ? d.run_status[lp] : LP_OPTIMAL;
    int status = run;
    int nseg = 0;
    if (run == LP_OPTIMAL) {
        int bad = 0;
        for (int t = tid; t < m; t += NT)
            if (N[t] < 0 || N[t] >= n) bad = 1;
        if (block_any(bad)) status = LP_BAD_ARG;
    }
    if (status == LP_OPTIMAL) {
        // ---- T = [A | b; c | 0; g | 0]; slots = the columns in order, basis = the artificials by row
        for (int s = tid; s < n; s += NT) slotvar[s] = s;
        for (int t = tid; t < m; t += NT) basis[t] = n + t;
        for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
            const int s = e / m, i = e - s * m;
            T[(size_t)i * pitch + s] = A[e];
        }
        for (int i = tid; i < m; i += NT) T[(size_t)i * pitch + n] = b[i];
        for (int j = tid; j < W; j += NT) {
            T[(size_t)m * pitch + j] = (j < n) ? c[j] : 0.0;
            T[(size_t)(m + 1) * pitch + j] = (j < n) ? g[j] : 0.0;
        }
        // the crash is skipped when the basis columns are the unit vectors in order and both costs are zero there
        int not_identity = 0;
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m;
            if (A[(size_t)N[t] * m + i] != ((i == t) ? 1.0 : 0.0)) not_identity = 1;
        }
        for (int t = tid; t < m; t += NT)
            if (c[N[t]] != 0.0 || g[N[t]] != 0.0) not_identity = 1;
        const bool identity = !block_any(not_identity);

        // ---- one Gauss-Jordan pivot on (row r, slot se) over all m+2 rows with tableau_pivot's arithmetic
        // (batched_lds_loop.hpp's, one row further); slot se receives the leaving variable's column.  All threads.
        const int G = NT / W > 0 ? NT / W : 1;   // row groups: a thread owns one column and every G-th row
        auto pivot = [&](int r, int se) {
            const double ur = T[(size_t)r * pitch + se];
            for (int j = tid; j < W; j += NT) prow[j] = T[(size_t)r * pitch + j];
            for (int i = tid; i <= m + 1; i += NT) lcol[i] = (i == r) ? 1.0 / ur : -T[(size_t)i * pitch + se] / ur;
            __syncthreads();
            for (int slot = tid; slot < G * W; slot += NT) {
                const int j = slot % W, gr = slot / W;
                const double pj = prow[j];
                for (int i = gr; i <= m + 1; i += G) {
                    const double l = lcol[i];
                    double* e = T + (size_t)i * pitch + j;
                    *e = (j == se) ? l : (i == r) ? pj * l : fma(l, pj, *e);
                }
            }
            if (tid == 0) {
                const int ve = slotvar[se];
                slotvar[se] = basis[r];
                basis[r] = ve;
            }
            __syncthreads();
        };
#include "batched_resolve_crash.hpp"

        const double* drow = T + (size_t)m * pitch;
        const double* grow = T + (size_t)(m + 1) * pitch;
        if (status == LP_OPTIMAL) {
            // ---- start check: primal and dual feasible at t = 0
            constexpr bool maximize = MX;
#include "batched_resolve_classify.hpp"
            if (!primal_feasible || !dual_feasible) status = LP_BAD_ARG;
        }
        if (status == LP_OPTIMAL) {
            // ---- the segments: wave 0 selects (tk, tend, zk, sk wave-uniform; lane 0 writes the records)
            double tk = 0.0, tend = 0.0, zk = 0.0, sk = 0.0;
            int k = 0, code = kGoOn;
            for (;; ++k) {
                if (wave == 0) {
                    if (lane == 0) {
                        double z = 0.0, s = 0.0;
                        for (int t = 0; t < m; ++t) {
                            const double gb = g[basis[t]], xb = T[(size_t)t * pitch + n];
                            z = fma(fma(tk, gb, c[basis[t]]), xb, z);
                            s = fma(gb, xb, s);
                        }
                        zk = z;
                        sk = s;
                        t_out[k] = tk;
                        obj_out[k] = z;
                        slope_out[k] = s;
                    }
                    // tau over the non-basic columns, keyed by variable: take keeps the first minimum
                    double bv = 0.0;
                    int bk = -1;
                    for (int s = lane; s < n; s += 64) {
                        const int v = slotvar[s];
                        const double dl = grow[s];
                        if (v < n && (MX ? (dl > eps) : (dl < -eps))) take<false>(-drow[s] / dl, v, bv, bk);
                    }
                    wave_take<false>(bv, bk);
                    const double ts = bv > tk ? bv : tk;
                    int se0 = -1, r = -1, cd = kGoOn;
                    if (bk < 0 || ts >= d.t_max) {
                        cd = kEndTMax;
                        tend = d.t_max;
                    } else {
                        int ls = INT_MAX;   // the slot that holds column bk
                        for (int s = lane; s < n; s += 64)
                            if (slotvar[s] == bk) ls = s;
                        se0 = lpdev::wave_min_i32(ls);
                        // tableau_loop's ratio test over slot se0 (the re-solve's primal loop, code for code)
                        const int se = se0;
                        int any_pos = 0;
                        if (m <= 128) {
                            double rv[2];
#pragma unroll
                            for (int q = 0; q < 2; ++q) {
                                const int i = lane + 64 * q;
                                const double ui = (i < m) ? T[(size_t)i * pitch + se] : 0.0;
                                rv[q] = (i < m && ui > eps) ? T[(size_t)i * pitch + n] / ui : INFINITY;
                                if (i < m && !(ui <= eps)) any_pos = 1;
                            }
                            r = wave_ratio_select<2>(rv, m, eps);
                        } else if (m <= 256) {
                            double rv[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int i = lane + 64 * q;
                                const double ui = (i < m) ? T[(size_t)i * pitch + se] : 0.0;
                                rv[q] = (i < m && ui > eps) ? T[(size_t)i * pitch + n] / ui : INFINITY;
                                if (i < m && !(ui <= eps)) any_pos = 1;
                            }
                            r = wave_ratio_select<4>(rv, m, eps);
                        } else {
                            for (int i = lane; i < m; i += 64)
                                if (!(T[(size_t)i * pitch + se] <= eps)) any_pos = 1;
                            double theta;
                            auto getr = [&](int i, double& v, int& key, bool& ok) {
                                const double ui = T[(size_t)i * pitch + se];
                                v = (ui > eps) ? T[(size_t)i * pitch + n] / ui : INFINITY;
                                key = i;
                                ok = true;
                            };
                            r = wave_scan_keyed<false>(m, eps, theta, getr);
                        }
                        if (!__any(any_pos)) r = -1;
                        tend = ts;
                        cd = r < 0 ? kEndUnbounded : k == MB ? kEndLimit : kGoOn;
                        if (lane == 0) {
                            enter_out[k] = bk;
                            if (cd == kGoOn) leave_out[k] = basis[r];
                        }
                    }
                    tk = ts;
                    if (lane == 0) {
                        pub[0] = se0;
                        pub[1] = r;
                        pub[2] = cd;
                    }
                }
                __syncthreads();
                const int se = pub[0], r = pub[1];
                code = pub[2];
                if (code != kGoOn) break;
                pivot(r, se);
            }
            nseg = k + 1;
            status = parametric_cost_status(code);
            if (tid == 0) {   // the last segment's end, with the last basis
                leave_out[k] = -1;
                if (code == kEndTMax) enter_out[k] = -1;
                t_out[k + 1] = tend;
                obj_out[k + 1] = tend == INFINITY ? (sk == 0.0 ? zk : sk > 0.0 ? INFINITY : -INFINITY) : value_at(tend);
            }
        }
    }
    // ---- outputs past the path: NaN / -1; the final basis (the given one without a path)
    for (int j = (nseg ? nseg + 1 : 0) + tid; j < MB + 2; j += NT) {
        t_out[j] = NAN;
        obj_out[j] = NAN;
    }
    for (int j = nseg + tid; j < MB + 1; j += NT) {
        slope_out[j] = NAN;
        enter_out[j] = -1;
        leave_out[j] = -1;
    }
    for (int t = tid; t < m; t += NT) d.basis_out[(size_t)lp * m + t] = nseg ? basis[t] : N[t];
    if (tid == 0) {
        d.nseg[lp] = nseg;
        d.status[lp] = status;
    }
}

// ---- the single-LP path beyond lp_basis_parametric_cost_fits

// Device scratch of one single-LP path.
struct CostRun {
    double tk;       // the current segment's start
    int k;           // pivots done
    int identity;    // k_pc_identity: the slack identity with zero c_B and g_B (the crash is skipped)
};
struct CostOut {
    const double* c;   // the costs (n)
    const double* g;   // the cost direction (n)
    double t_max;
    int max_breaks;
    int* nseg;
    double *t, *obj, *slope;
    int *enter, *leave;
};

// Rows 0..m of T (pitch ld) = [A | b; cost | 0]: column n is the right-hand side
__global__ __launch_bounds__(256) void k_pc_gather(SimplexDev s, const double* A, const double* b,
                                                   const double* cost) {
    const int i = blockIdx.x;   // tableau row, 0..m
    const int m = s.m, n = s.n;
    double* row = s.T + (size_t)i * s.ld;
    for (int j = threadIdx.x; j < s.ld; j += blockDim.x) {
        double v = 0.0;
        if (i == m) v = j < n ? cost[j] : 0.0;
        else if (j < n) v = A[(size_t)j * m + i];
        else if (j == n) v = b[i];
        row[j] = v;
    }
}

// One block: the basis and the non-basic flags, and the slack-identity test (zero c_B and g_B)
__global__ __launch_bounds__(256) void k_pc_identity(SimplexDev s, const double* A, const double* c,
                                                     const double* g, const int* basis, CostRun* run) {
    __shared__ int not_identity;
    const int m = s.m, n = s.n, tid = threadIdx.x;
    if (tid == 0) not_identity = 0;
    for (int j = tid; j < n; j += 256) s.nonbasic[j] = 1;
    __syncthreads();
    for (int t = tid; t < m; t += 256) {
        s.basis[t] = basis[t];
        s.nonbasic[basis[t]] = 0;
        if (c[basis[t]] != 0.0 || g[basis[t]] != 0.0) not_identity = 1;
    }
    for (int e = tid; e < m * m; e += 256) {
        const int t = e / m, i = e - t * m;
        if (A[(size_t)basis[t] * m + i] != ((i == t) ? 1.0 : 0.0)) not_identity = 1;
    }
    __syncthreads();
    if (tid == 0) run->identity = !not_identity;
}

// One block: the start check and the state word (kRunning, or LP_BAD_ARG for a basis that is not optimal at t = 0)
template <bool MX>
__global__ __launch_bounds__(1024) void k_pc_begin(SimplexDev s, double eps, CostRun* run) {
    const int tid = threadIdx.x, m = s.m, n = s.n, ld = s.ld;
    int pinf = 0, dinf = 0;
    for (int i = tid; i < m; i += blockDim.x)
        if (s.T[(size_t)i * ld + n] < -eps) pinf = 1;
    const double* drow = s.T + (size_t)m * ld;
    for (int j = tid; j < n; j += blockDim.x)
        if (s.nonbasic[j] && (MX ? (drow[j] > eps) : (drow[j] < -eps))) dinf = 1;
    pinf = __syncthreads_or(pinf);
    dinf = __syncthreads_or(dinf);
    if (tid == 0) {
        SimplexState* st = s.state;
        st->status = (pinf || dinf) ? LP_BAD_ARG : kRunning;
        st->iters = 0;
        st->max_iter = 0;
        st->enter = st->leave = -1;
        st->pivot_valid = 0;
        st->eps = eps;
        run->tk = 0.0;
        run->k = 0;
    }
}

// One breakpoint (one workgroup): wave 0 writes the segment record, reduces tau and runs the primal ratio test; then
// the block stages the pivot over all m+2 rows for k_simplex_update, or lane 0 closes the path.
template <bool MX>
__global__ __launch_bounds__(1024) void k_pc_select(SimplexDev s, CostOut o, CostRun* run) {
    SimplexState* st = s.state;
    __shared__ int s_pick[3];   // leaving position, entering column, end code
    const int tid = threadIdx.x;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = s.m, n = s.n, ld = s.ld;
    const double eps = st->eps;
    const double* T = s.T;
    if (tid < 64) {
        const int lane = tid;
        const int k = run->k;
        const double tk = run->tk;
        auto value_at = [&](double tt) {
            double z = 0.0;
            for (int t = 0; t < m; ++t)
                z = fma(fma(tt, o.g[s.basis[t]], o.c[s.basis[t]]), T[(size_t)t * ld + n], z);
            return z;
        };
        double zk = 0.0, sk = 0.0;
        if (lane == 0) {
            double sl = 0.0;
            for (int t = 0; t < m; ++t) sl = fma(o.g[s.basis[t]], T[(size_t)t * ld + n], sl);
            zk = value_at(tk);
            sk = sl;
            o.t[k] = tk;
            o.obj[k] = zk;
            o.slope[k] = sk;
        }
        const double* drow = T + (size_t)m * ld;
        const double* grow = T + (size_t)(m + 1) * ld;
        double bv = 0.0;
        int bk = -1;
        for (int j = lane; j < n; j += 64) {   // j ascending per lane: take keeps the first minimum
            const double dl = grow[j];
            if (s.nonbasic[j] && (MX ? (dl > eps) : (dl < -eps))) take<false>(-drow[j] / dl, j, bv, bk);
        }
        wave_take<false>(bv, bk);
        const double ts = bv > tk ? bv : tk;
        int r = -1, code = kGoOn;
        double tend = o.t_max;
        if (bk < 0 || ts >= o.t_max) {
            code = kEndTMax;
        } else {
            int any_pos = 0;
            for (int i = lane; i < m; i += 64)
                if (!(T[(size_t)i * ld + bk] <= eps)) any_pos = 1;
            double best;
            auto load_r = [&](int i, bool& ok) {
                const double ui = T[(size_t)i * ld + bk];
                ok = ui > eps;
                return T[(size_t)i * ld + n] / ui;
            };
            r = lpdev::wave_chain_select<false>(m, eps, best, load_r);
            if (!__any(any_pos)) r = -1;
            tend = ts;
            code = r < 0 ? kEndUnbounded : k == o.max_breaks ? kEndLimit : kGoOn;
            if (lane == 0) {
                o.enter[k] = bk;
                if (code == kGoOn) o.leave[k] = s.basis[r];
            }
        }
        if (lane == 0) {
            if (code != kGoOn) {   // the last segment's end, with the last basis
                o.leave[k] = -1;
                if (code == kEndTMax) o.enter[k] = -1;
                o.t[k + 1] = tend;
                o.obj[k + 1] = tend == INFINITY ? (sk == 0.0 ? zk : sk > 0.0 ? INFINITY : -INFINITY) : value_at(tend);
                *o.nseg = k + 1;
                st->status = parametric_cost_status(code);
                st->pivot_valid = 0;
            } else {
                run->tk = ts;
                run->k = k + 1;
            }
            s_pick[0] = r;
            s_pick[1] = bk;
            s_pick[2] = code;
        }
    }
    __syncthreads();
    if (s_pick[2] != kGoOn) return;
    const int r = s_pick[0], e = s_pick[1];
    const double ur = T[(size_t)r * ld + e];
    for (int i = tid; i <= m + 1; i += blockDim.x) s.lcol[i] = (i == r) ? 1.0 / ur : -T[(size_t)i * ld + e] / ur;
    for (int j = tid; j < ld; j += blockDim.x) s.prow[j] = T[(size_t)r * ld + j];
    if (tid == 0) {
        const int old = s.basis[r];
        s.basis[r] = e;
        s.nonbasic[e] = 0;
        s.nonbasic[old] = 1;
        st->iters = st->iters + 1;
        st->enter = e;
        st->leave = r;
        st->pivot_valid = 1;
    }
}

}  // namespace

size_t lp_basis_parametric_cost_lds_bytes(int m, int n, int* pitch_out) {
    const int W = n + 1;
    const int pitch = (W & 1) ? W : W + 1;   // odd pitch: conflict-free column reads
    if (pitch_out) *pitch_out = pitch;
    const size_t dbl = sizeof(Published) / 8 + (size_t)(m + 2) * pitch + W + (m + 2);
    const size_t bytes = dbl * 8 + sizeof(int) * ((size_t)n + m);
    return (bytes + 15) & ~(size_t)15;
}

int lp_basis_parametric_cost_launch(lp_context* ctx, const BasisParametricDev& d, int maximize) {
    if (!lp_basis_parametric_cost_fits(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "basis parametric cost: the shape does not fit one CU's LDS");
    if (d.batch <= 0) return LP_OPTIMAL;
    const size_t cells = (size_t)(d.m + 1) * (d.n + 1), shm = lp_basis_parametric_cost_lds_bytes(d.m, d.n, nullptr);
    if (maximize)
        return lp_launch_per_lp(ctx, cells, k_batched_parametric_cost<256, true>, k_batched_parametric_cost<1024, true>,
                                shm, d);
    return lp_launch_per_lp(ctx, cells, k_batched_parametric_cost<256, false>, k_batched_parametric_cost<1024, false>,
                            shm, d);
}

// One LP of any size on the device: A, b, c, g, basis already there (ranges checked by the caller).
int lp_basis_parametric_cost_device(lp_context* ctx, const double* dA, int m, int n, const double* db,
                                    const double* dc, const int* dbasis, const double* dg, int maximize, double t_max,
                                    double eps, int max_breaks, int* dnseg, double* dt, double* dobj, double* dslope,
                                    int* denter, int* dleave, int* dbasis_out) {
    hipStream_t s = ctx->stream;
    const int ld = (int)lp_ceil_div<size_t>((size_t)n + 1, 8) * 8;
    const size_t row_bytes = sizeof(double) * (size_t)ld;
    lp_simplex_problem q;   // the crash's view: m constraint rows, the cost row m
    q.ctx = ctx;
    q.tableau_bytes = row_bytes * (size_t)(m + 1);
    SimplexDev& sd = q.dev;
    sd.m = m;
    sd.n = n;
    sd.ld = ld;
    sd.maximize = maximize ? 1 : 0;
    // one allocation: T (m+2 rows), the crash's permutation buffer (m+1 rows), lcol (m+2), prow, state, basis,
    // rowpos, rowused, nonbasic, the run record
    CostRun* run;
    auto pieces = [&](lp_carver& cv) {
        sd.T = cv.take<double>(row_bytes * (size_t)(m + 2));
        q.dT0 = cv.take<double>(q.tableau_bytes);
        sd.lcol = cv.take<double>(sizeof(double) * ((size_t)m + 2));
        sd.prow = cv.take<double>(row_bytes);
        sd.state = cv.take<SimplexState>(sizeof(SimplexState));
        sd.basis = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowpos = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowused = cv.take<unsigned char>((size_t)m);
        sd.nonbasic = cv.take<unsigned char>((size_t)n);
        run = cv.take<CostRun>(sizeof(CostRun));
    };
    char* arena = nullptr;
    LP_HIP(ctx, lp_carve_malloc(&arena, pieces));
    lp_simplex_problem qv;   // the update's view: rows 0..m+1 (m+1 "constraint" rows and the g row)
    qv.ctx = ctx;
    qv.dev = sd;
    qv.dev.m = m + 1;
    CostOut o{dc, dg, t_max, max_breaks, dnseg, dt, dobj, dslope, denter, dleave};
    double* grow = sd.T + (size_t)(m + 1) * ld;
    SimplexState* hstate = nullptr;
    int rc = LP_OPTIMAL;
    hipError_t e = hipHostMalloc(&hstate, sizeof(SimplexState));
    if (e == hipSuccess) {
        q.h_state = hstate;
        CostRun hr{};
        // rows 0..m = [A | b; g | 0] first: the crash (when it runs) leaves delta in row m, which moves to row m+1
        hipLaunchKernelGGL(k_pc_gather, m + 1, 256, 0, s, sd, dA, db, dg);
        hipLaunchKernelGGL(k_pc_identity, 1, 256, 0, s, sd, dA, dc, dg, dbasis, run);
        e = hipMemcpyAsync(&hr, run, sizeof(hr), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess && !hr.identity)
            rc = lp_simplex_crash(&q);   // m launch pairs, the verdict, rows into position order; one host sync
        if (e == hipSuccess && rc == LP_OPTIMAL) {
            e = hipMemcpyAsync(grow, sd.T + (size_t)m * ld, row_bytes, hipMemcpyDeviceToDevice, s);
            // then [A | b; c | 0] through the same crash: rows 0..m-1 come out as they did with g in row m
            if (e == hipSuccess) hipLaunchKernelGGL(k_pc_gather, m + 1, 256, 0, s, sd, dA, db, dc);
            if (e == hipSuccess && !hr.identity) rc = lp_simplex_crash(&q);
        }
        if (e == hipSuccess && rc == LP_OPTIMAL) {
            if (maximize)
                hipLaunchKernelGGL(k_pc_begin<true>, 1, 1024, 0, s, sd, eps, run);
            else
                hipLaunchKernelGGL(k_pc_begin<false>, 1, 1024, 0, s, sd, eps, run);
            rc = lp_poll_pivots(&q, [&](int batch) {
                for (int k = 0; k < batch; ++k) {
                    if (maximize)
                        hipLaunchKernelGGL(k_pc_select<true>, 1, 1024, 0, s, sd, o, run);
                    else
                        hipLaunchKernelGGL(k_pc_select<false>, 1, 1024, 0, s, sd, o, run);
                    lp_simplex_launch_update(&qv);
                }
                return 2 * batch;
            });
            if (rc == LP_OPTIMAL) {
                rc = hstate->status;
                if (rc != LP_BAD_ARG) e = hipMemcpyAsync(dbasis_out, sd.basis, sizeof(int) * (size_t)m,
                                                         hipMemcpyDeviceToDevice, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
            }
        }
    }
    if (e != hipSuccess) {
        ctx->last_error = std::string("basis parametric cost: ") + hipGetErrorString(e);
        rc = -(int)e;
    }
    if (hstate) (void)hipHostFree(hstate);
    (void)hipFree(arena);
    return rc;
}
