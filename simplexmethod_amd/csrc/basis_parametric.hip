// basis_parametric.hip — the parametric right-hand-side path z*(t) = opt { c.x : A x = b + t d, x >= 0 } from a given
// optimal basis, for t from 0 up to t_max, exactly as tests/ref/parametric_ref.c states it:
//   - install the basis: the re-solve's crash on [A | b | d] (batched_resolve_crash.hpp); the d column is updated
//     like every other column, so beta = B^-1 b and delta = B^-1 d are tableau columns;
//   - start check: no beta_t < -eps and no non-basic d_j > eps (max) / d_j < -eps (min), else LP_BAD_ARG;
//   - per segment k (from t_k): obj = the chain fma(c_B, fma(t_k, delta, beta), s) and slope = the chain
//     fma(c_B, delta, s) in position order, on one lane; the breakpoint is the first strict minimum of
//     tau_t = -beta_t / delta_t over delta_t < -eps (basis_crash.hpp's take), t* = max(tau, t_k); then the dual
//     entering chain over row r (the re-solve's), and one pivot.  The path ends at t_max (LP_OPTIMAL), at t* with
//     no entering column (LP_INFEASIBLE) or at t* after max_breaks pivots (LP_ITER_LIMIT).
//
// k_batched_parametric<NT, MX>: one LP per workgroup, the (m+1) x pitch tableau in LDS in batched_resolve.hip's
// layout with two right-hand columns (b in slot n, d in slot n+1).  The sense is a template parameter (DESIGN
// §4.5e: with a run-time flag selecting the comparison, -O3 reductions returned wrong winners on gfx950).
//
// Shapes beyond lp_basis_parametric_fits: k_param_gather builds [A | d | b; c | 0 | 0] with the d column barred from
// entering, lp_simplex_crash installs the basis, k_param_begin checks the start, then k_param_select<MX> (one
// workgroup: the segment record, the tau reduction and the dual entering chain of device_select.hpp) and the
// existing k_simplex_update run once per breakpoint, queued in batches under the polling loop.
#include <cfloat>

#include "basis_crash.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"
#include "device_select.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kRunning = -100;   // SimplexState::status while pivoting
enum { kGoOn = 0, kEndTMax = 1, kEndInfeasible = 2, kEndLimit = 3 };

__host__ __device__ inline int parametric_status(int code) {
    return code == kEndInfeasible ? LP_INFEASIBLE : code == kEndLimit ? LP_ITER_LIMIT : LP_OPTIMAL;
}

template <int NT, bool MX>
__global__ __launch_bounds__(NT) void k_batched_parametric(BasisParametricDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int m = d.m, n = d.n, W = n + 2, pitch = d.pitch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve (batched_resolve.hip's, two right-hand columns)
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = smem + sizeof(Published) / 8;             // (m+1) x pitch
    double* prow = T + (size_t)(m + 1) * pitch;           // W
    double* lcol = prow + W;                              // m+1
    int* slotvar = reinterpret_cast<int*>(lcol + m + 1);  // n
    int* basis = slotvar + n;                             // m
    int* pub = pubs->v;   // [0] entering slot / crash row, [1] leaving position, [2] verdict / end code, [3] block_any

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* dv = d.dir + (size_t)lp * m;
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
    // sum_t c[basis[t]] * fma(tt, delta_t, beta_t), the chain in position order (one lane)
    auto value_at = [&](double tt) {
        double s = 0.0;
        for (int t = 0; t < m; ++t)
            s = fma(c[basis[t]], fma(tt, T[(size_t)t * pitch + n + 1], T[(size_t)t * pitch + n]), s);
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
        // ---- T = [A | b | d; c | 0 | 0]; slots = the columns in order, basis = the artificials by row
        for (int s = tid; s < n; s += NT) slotvar[s] = s;
        for (int t = tid; t < m; t += NT) basis[t] = n + t;
        for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
            const int s = e / m, i = e - s * m;
            T[(size_t)i * pitch + s] = A[e];
        }
        for (int i = tid; i < m; i += NT) {
            T[(size_t)i * pitch + n] = b[i];
            T[(size_t)i * pitch + n + 1] = dv[i];
        }
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

        // ---- pivot(r, se) (the primal loop of the include is not used)
        constexpr bool BLAND = false;
#include "batched_lds_loop.hpp"
        (void)simplex;
#include "batched_resolve_crash.hpp"

        const double* drow = T + (size_t)m * pitch;
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
                            const double cb = c[basis[t]], de = T[(size_t)t * pitch + n + 1];
                            z = fma(cb, fma(tk, de, T[(size_t)t * pitch + n]), z);
                            s = fma(cb, de, s);
                        }
                        zk = z;
                        sk = s;
                        t_out[k] = tk;
                        obj_out[k] = z;
                        slope_out[k] = s;
                    }
                    double bv = 0.0;
                    int bk = -1;
                    for (int t = lane; t < m; t += 64) {   // t ascending per lane: take keeps the first minimum
                        const double de = T[(size_t)t * pitch + n + 1];
                        if (de < -eps) take<false>(-T[(size_t)t * pitch + n] / de, t, bv, bk);
                    }
                    wave_take<false>(bv, bk);
                    const double ts = bv > tk ? bv : tk;
                    int se0 = -1, cd = kGoOn;
                    if (bk < 0 || ts >= d.t_max) {
                        cd = kEndTMax;
                        tend = d.t_max;
                    } else {
                        const double* rrow = T + (size_t)bk * pitch;
                        double best;
                        se0 = wave_scan_keyed<false>(n, eps, best, [&](int s, double& v, int& key, bool& ok) {
                            const double a = rrow[s];
                            key = slotvar[s];
                            ok = key < n && a < -eps;
                            v = MX ? drow[s] / a : -drow[s] / a;
                        });
                        tend = ts;
                        cd = se0 < 0 ? kEndInfeasible : k == MB ? kEndLimit : kGoOn;
                        if (lane == 0) {
                            leave_out[k] = basis[bk];
                            if (cd == kGoOn) enter_out[k] = slotvar[se0];
                        }
                    }
                    tk = ts;
                    if (lane == 0) {
                        pub[0] = se0;
                        pub[1] = bk;
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
            status = parametric_status(code);
            if (tid == 0) {   // the last segment's end, with the last basis
                enter_out[k] = -1;
                if (code == kEndTMax) leave_out[k] = -1;
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

// ---- the single-LP path beyond lp_basis_parametric_fits

// Device scratch and outputs of one single-LP path.
struct ParamRun {
    double tk;       // the current segment's start
    int k;           // pivots done
    int identity;    // k_param_identity: the slack identity with zero costs (the crash is skipped)
};
struct ParamOut {
    const double* c;   // the costs (n)
    double t_max;
    int max_breaks;
    int* nseg;
    double *t, *obj, *slope;
    int *enter, *leave;
};

// T (m+1 rows, pitch ld) = [A | d | b; c | 0 | 0]: column n is the direction, column n+1 = s.n the right-hand side
__global__ __launch_bounds__(256) void k_param_gather(SimplexDev s, const double* A, int n, const double* b,
                                                      const double* c, const double* dir) {
    const int i = blockIdx.x;   // tableau row, 0..m
    const int m = s.m;
    double* row = s.T + (size_t)i * s.ld;
    for (int j = threadIdx.x; j < s.ld; j += blockDim.x) {
        double v = 0.0;
        if (i == m) v = j < n ? c[j] : 0.0;
        else if (j < n) v = A[(size_t)j * m + i];
        else if (j == n) v = dir[i];
        else if (j == n + 1) v = b[i];
        row[j] = v;
    }
}

// One block: the basis and the non-basic flags (the d column barred), and the slack-identity test
__global__ __launch_bounds__(256) void k_param_identity(SimplexDev s, const double* A, int n, const double* c,
                                                        const int* basis, ParamRun* run) {
    __shared__ int not_identity;
    const int m = s.m, tid = threadIdx.x;
    if (tid == 0) not_identity = 0;
    for (int j = tid; j <= n; j += 256) s.nonbasic[j] = j < n ? 1 : 0;
    __syncthreads();
    for (int t = tid; t < m; t += 256) {
        s.basis[t] = basis[t];
        s.nonbasic[basis[t]] = 0;
        if (c[basis[t]] != 0.0) not_identity = 1;
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
__global__ __launch_bounds__(1024) void k_param_begin(SimplexDev s, int n, double eps, ParamRun* run) {
    const int tid = threadIdx.x, m = s.m, ld = s.ld;
    int pinf = 0, dinf = 0;
    for (int i = tid; i < m; i += blockDim.x)
        if (s.T[(size_t)i * ld + n + 1] < -eps) pinf = 1;
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

// One breakpoint (one workgroup): wave 0 writes the segment record, reduces tau and runs the dual entering chain;
// then the block stages the pivot for k_simplex_update, or lane 0 closes the path.
template <bool MX>
__global__ __launch_bounds__(1024) void k_param_select(SimplexDev s, int n, ParamOut o, ParamRun* run) {
    SimplexState* st = s.state;
    __shared__ int s_pick[3];   // leaving position, entering column, end code
    const int tid = threadIdx.x;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = s.m, ld = s.ld;
    const double eps = st->eps;
    const double* T = s.T;
    if (tid < 64) {
        const int lane = tid;
        const int k = run->k;
        const double tk = run->tk;
        auto value_at = [&](double tt) {
            double z = 0.0;
            for (int t = 0; t < m; ++t)
                z = fma(o.c[s.basis[t]], fma(tt, T[(size_t)t * ld + n], T[(size_t)t * ld + n + 1]), z);
            return z;
        };
        double zk = 0.0, sk = 0.0;
        if (lane == 0) {
            double sl = 0.0;
            for (int t = 0; t < m; ++t) sl = fma(o.c[s.basis[t]], T[(size_t)t * ld + n], sl);
            zk = value_at(tk);
            sk = sl;
            o.t[k] = tk;
            o.obj[k] = zk;
            o.slope[k] = sk;
        }
        double bv = 0.0;
        int bk = -1;
        for (int t = lane; t < m; t += 64) {
            const double de = T[(size_t)t * ld + n];
            if (de < -eps) take<false>(-T[(size_t)t * ld + n + 1] / de, t, bv, bk);
        }
        wave_take<false>(bv, bk);
        const double ts = bv > tk ? bv : tk;
        int e = -1, code = kGoOn;
        double tend = o.t_max;
        if (bk < 0 || ts >= o.t_max) {
            code = kEndTMax;
        } else {
            const double* trow = T + (size_t)bk * ld;
            const double* drow = T + (size_t)m * ld;
            double best;
            auto load_q = [&](int j, bool& ok) {
                const double a = trow[j];
                ok = s.nonbasic[j] != 0 && a < -eps;
                return MX ? drow[j] / a : -drow[j] / a;
            };
            e = lpdev::wave_chain_select<false>(n, eps, best, load_q);
            tend = ts;
            code = e < 0 ? kEndInfeasible : k == o.max_breaks ? kEndLimit : kGoOn;
            if (lane == 0) {
                o.leave[k] = s.basis[bk];
                if (code == kGoOn) o.enter[k] = e;
            }
        }
        if (lane == 0) {
            if (code != kGoOn) {   // the last segment's end, with the last basis
                o.enter[k] = -1;
                if (code == kEndTMax) o.leave[k] = -1;
                o.t[k + 1] = tend;
                o.obj[k + 1] = tend == INFINITY ? (sk == 0.0 ? zk : sk > 0.0 ? INFINITY : -INFINITY) : value_at(tend);
                *o.nseg = k + 1;
                st->status = parametric_status(code);
                st->pivot_valid = 0;
            } else {
                run->tk = ts;
                run->k = k + 1;
            }
            s_pick[0] = bk;
            s_pick[1] = e;
            s_pick[2] = code;
        }
    }
    __syncthreads();
    if (s_pick[2] != kGoOn) return;
    const int r = s_pick[0], e = s_pick[1];
    const double ur = T[(size_t)r * ld + e];
    for (int i = tid; i <= m; i += blockDim.x) s.lcol[i] = (i == r) ? 1.0 / ur : -T[(size_t)i * ld + e] / ur;
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

size_t lp_basis_parametric_lds_bytes(int m, int n, int* pitch_out) {
    const int W = n + 2;
    const int pitch = (W & 1) ? W : W + 1;   // odd pitch: conflict-free column reads
    if (pitch_out) *pitch_out = pitch;
    const size_t dbl = sizeof(Published) / 8 + (size_t)(m + 1) * pitch + W + (m + 1);
    const size_t bytes = dbl * 8 + sizeof(int) * ((size_t)n + m);
    return (bytes + 15) & ~(size_t)15;
}

int lp_basis_parametric_launch(lp_context* ctx, const BasisParametricDev& d, int maximize) {
    if (!lp_basis_parametric_fits(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "basis parametric: the shape does not fit one CU's LDS");
    if (d.batch <= 0) return LP_OPTIMAL;
    const size_t cells = (size_t)(d.m + 1) * (d.n + 1), shm = lp_basis_parametric_lds_bytes(d.m, d.n, nullptr);
    if (maximize)
        return lp_launch_per_lp(ctx, cells, k_batched_parametric<256, true>, k_batched_parametric<1024, true>, shm, d);
    return lp_launch_per_lp(ctx, cells, k_batched_parametric<256, false>, k_batched_parametric<1024, false>, shm, d);
}

// One LP of any size on the device: A, b, c, d, basis already there (ranges checked by the caller).
int lp_basis_parametric_device(lp_context* ctx, const double* dA, int m, int n, const double* db, const double* dc,
                               const int* dbasis, const double* ddir, int maximize, double t_max, double eps,
                               int max_breaks, int* dnseg, double* dt, double* dobj, double* dslope, int* denter,
                               int* dleave, int* dbasis_out) {
    hipStream_t s = ctx->stream;
    const int ld = (int)lp_ceil_div<size_t>((size_t)n + 2, 8) * 8;
    lp_simplex_problem q;
    q.ctx = ctx;
    q.tableau_bytes = sizeof(double) * (size_t)(m + 1) * ld;
    SimplexDev& sd = q.dev;
    sd.m = m;
    sd.n = n + 1;   // [A | d] as n+1 columns, b in column n+1
    sd.ld = ld;
    sd.maximize = maximize ? 1 : 0;
    // one allocation: T, the pristine copy the crash permutes through, lcol, prow, state, basis, rowpos, rowused,
    // nonbasic, the run record
    ParamRun* run;
    auto pieces = [&](lp_carver& cv) {
        sd.T = cv.take<double>(q.tableau_bytes);
        q.dT0 = cv.take<double>(q.tableau_bytes);
        sd.lcol = cv.take<double>(sizeof(double) * ((size_t)m + 1));
        sd.prow = cv.take<double>(sizeof(double) * (size_t)ld);
        sd.state = cv.take<SimplexState>(sizeof(SimplexState));
        sd.basis = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowpos = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowused = cv.take<unsigned char>((size_t)m);
        sd.nonbasic = cv.take<unsigned char>((size_t)n + 1);
        run = cv.take<ParamRun>(sizeof(ParamRun));
    };
    char* arena = nullptr;
    LP_HIP(ctx, lp_carve_malloc(&arena, pieces));
    ParamOut o{dc, t_max, max_breaks, dnseg, dt, dobj, dslope, denter, dleave};
    SimplexState* hstate = nullptr;
    int rc = LP_OPTIMAL;
    hipError_t e = hipHostMalloc(&hstate, sizeof(SimplexState));
    if (e == hipSuccess) {
        q.h_state = hstate;
        ParamRun hr{};
        hipLaunchKernelGGL(k_param_gather, m + 1, 256, 0, s, sd, dA, n, db, dc, ddir);
        hipLaunchKernelGGL(k_param_identity, 1, 256, 0, s, sd, dA, n, dc, dbasis, run);
        e = hipMemcpyAsync(&hr, run, sizeof(hr), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess && !hr.identity)
            rc = lp_simplex_crash(&q);   // m launch pairs, the verdict, rows into position order; one host sync
        if (e == hipSuccess && rc == LP_OPTIMAL) {
            if (maximize)
                hipLaunchKernelGGL(k_param_begin<true>, 1, 1024, 0, s, sd, n, eps, run);
            else
                hipLaunchKernelGGL(k_param_begin<false>, 1, 1024, 0, s, sd, n, eps, run);
            rc = lp_poll_pivots(&q, [&](int batch) {
                for (int k = 0; k < batch; ++k) {
                    if (maximize)
                        hipLaunchKernelGGL(k_param_select<true>, 1, 1024, 0, s, sd, n, o, run);
                    else
                        hipLaunchKernelGGL(k_param_select<false>, 1, 1024, 0, s, sd, n, o, run);
                    lp_simplex_launch_update(&q);
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
        ctx->last_error = std::string("basis parametric: ") + hipGetErrorString(e);
        rc = -(int)e;
    }
    if (hstate) (void)hipHostFree(hstate);
    (void)hipFree(arena);
    return rc;
}
