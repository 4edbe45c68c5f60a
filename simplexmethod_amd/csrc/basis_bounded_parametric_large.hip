// basis_bounded_parametric_large.hip — the parametric right-hand-side path and the parametric cost path of ONE
// bounded-variable LP of any shape, on the tableau in HBM (lp_basis_bounded_parametric_large and
// lp_basis_bounded_parametric_cost_large).  The definition is tests/ref/bounded_parametric_ref.c (the step numbers
// below are its); basis_bounded_parametric.hip is the same path for shapes that fit one workgroup's LDS.
//
// Read simplex_bounded_launch.hip's header first: the full tableau (one column per variable, a basic column the exact
// unit vector) reproduces the reference's slot tableau bit for bit, and a complemented pivot row exists only in the
// staged copy the unchanged k_simplex_update reads.  BoundedLargeDev (U, up, the quotient scratch) is reused as it is.
//
// Setup (both paths): U and the flags (k_bparl_bounds), b' as the reference's two chains per row (k_bparl_bprime), the
// tableau on the shifted variables with every flagged column held complemented (k_bparl_gather), the basis, the
// non-basic flags and the identity test on the columns as loaded (k_bparl_identity), lp_simplex_crash unless that test
// passes, the start check of step 4 (k_bparl_begin).
//   RHS path   [A' | d | b'] as sd.n = n + 1 columns: d is column n, barred from entering, beta is column n + 1.  The
//              update carries both right-hand columns, and the staging rule of a complemented row
//              (j < sd.n ? -v : j == sd.n ? U - v : v) is R2's complement: delta_r negated, beta_r = U - beta_r.
//   cost path  m + 2 rows: row m holds c', row m + 1 holds g'.  ONE crash: behind each step's selector
//              k_bparl_second_eta stages the g' row's eta entry -g'_e / u_r, and the step's update runs on the view
//              with m + 1 "constraint" rows, so g' takes fma(l, prow_j, g'_j) and column e as every other row does.
//              The walk then uses the same view.
//
// One selector launch and one k_simplex_update launch per breakpoint, polled by lp_poll_pivots.  A selector
// (k_bparl_select_rhs / _cost, one workgroup of 1024 threads):
//   1. every thread gathers: per basis position the operands of the two chains of R3 / C3 into LDS (the cost entry,
//      the value x_t in the caller's variables at t_k, the slope operand), and its share of the tau candidates (the
//      first strict minimum, the first position or column on a tie: basis_crash.hpp's take);
//   2. one barrier; then the LAST WAVE runs the two chains (position order over LDS, then the held non-basic columns
//      with h_j != 0 in index order, 256 columns loaded at a time and the non-zero ones picked by ballot), writes t, obj
//      and slope of segment k, raises a flag in LDS and leaves the kernel;
//   3. meanwhile the other fifteen waves clamp t* = max(tau, t_k), decide the ends, run the entering chain over the
//      (complemented) row r (RHS) or the bounded ratio test over column e (cost) through lpdev::block_chain_select on
//      960 threads, write enter, leave and side, and stage lcol and prow, or flip the bound inside the selector;
//   4. thread 0 waits for the flag before it touches what the chain wave reads (the flags, the non-basic marks), so
//      the two meet at the end.  The chain wave waits for nobody.
// A workgroup barrier waits for every wave that has not left the kernel, so the first barrier of the scan (inside
// block_chain_select, behind its first pass) also waits for the chain wave's end: what runs beside the chains is the
// tau combination and the scan's first pass (the loads of row r and the cost row, or of column e and xB, and the
// divisions); the near-tie check and the staging follow it.
// A blocking row or column that ends the path leaves no trace.  obj[nseg] is k_bparl_finish's, once per call, with
// the same gather and the same chain at the path's end.
//
// Dynamic LDS (checked against 156 KiB as the other HBM selectors are): 24 m + 416 bytes (RHS), 40 m + 448 bytes
// (cost): m <= 6638 and m <= 3982.  n is bounded by device memory only.
//
// Plain C++ and vector stores only: no inline assembly and no scalar-memory writes in this file.
#include <cfloat>
#include <climits>

#include "basis_crash.hpp"
#include "batched_problem.hpp"
#include "device_select.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kRunning = -100;   // SimplexState::status while pivoting
constexpr int kScan = 960;       // the threads of a selector that are not the chain wave

struct BparlRun {
    double tk;     // the current segment's start
    double tend;   // the path's end, once it has ended
    int k;         // breakpoints passed
    int identity;  // k_bparl_identity: the unit basis in order with zero cost rows (the crash is skipped)
};

// What a selector needs beside the tableau and the bound state (by value)
struct BparlDev {
    int n;             // the LP's columns (the RHS tableau has one more)
    int max_breaks;
    double t_max;
    const double *c, *g;   // the caller's costs; the cost direction (cost path only)
    const double *lo, *hi;
    int* nseg;
    double *t, *obj, *slope;
    int *enter, *leave, *side;
    BparlRun* run;
};

// The per-selector LDS pieces both paths share
struct BparlLds {
    double *ca, *xa, *sa;            // m each: the chains' operands by position
    lpdev::BlockChainScratch* sc;
    double* tauv;                    // 16: the waves' tau candidates
    int* taui;                       // 16
    int* done;                       // the chain wave's flag
};

__host__ __device__ inline size_t bparl_lds_bytes(int m, bool cost) {
    return sizeof(double) * (3 * (size_t)m + (cost ? 2 * ((size_t)m + 2) : 0)) + sizeof(lpdev::BlockChainScratch) +
           16 * sizeof(double) + 16 * sizeof(int) + 16;
}

__device__ __forceinline__ BparlLds bparl_carve(double* base, int m) {
    BparlLds L;
    L.ca = base;
    L.xa = L.ca + m;
    L.sa = L.xa + m;
    L.sc = reinterpret_cast<lpdev::BlockChainScratch*>(L.sa + m);
    L.tauv = reinterpret_cast<double*>(L.sc + 1);
    L.taui = reinterpret_cast<int*>(L.tauv + 16);
    L.done = L.taui + 16;
    return L;
}

// ---- setup

// U = hi - lo and the flags per tableau column; the RHS path's d column gets +inf and no flag
__global__ __launch_bounds__(256) void k_bparl_bounds(int n, int cols, const double* lo, const double* hi,
                                                      const int* at_upper, double* U, int* up) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    U[j] = j < n ? hi[j] - lo[j] : INFINITY;
    up[j] = j < n ? at_upper[j] : 0;
}

// b' (bounded_resolve_ref.c steps 2-3): per row the chain over lo_j != 0, then over the flagged columns with U_j
__global__ __launch_bounds__(64) void k_bparl_bprime(const double* A, int m, int n, const double* b, const double* lo,
                                                     const double* U, const int* up, double* bp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double acc = b[i];
    for (int j = 0; j < n; ++j) {
        const double l = lo[j];
        if (l != 0.0) acc = fma(-A[(size_t)j * m + i], l, acc);
    }
    for (int j = 0; j < n; ++j)
        if (up[j]) acc = fma(-A[(size_t)j * m + i], U[j], acc);
    bp[i] = acc;
}

// The tableau, one block per row.  RHS: rows 0..m of [A' | d | b'; c' | 0 | 0]; cost: rows 0..m+1 of
// [A' | b'; c' | 0; g' | 0]; a flagged column changes sign in every row.
template <bool COST>
__global__ __launch_bounds__(256) void k_bparl_gather(SimplexDev s, int n, const double* A, const double* bp,
                                                      const double* c, const double* dir, const int* up) {
    const int i = blockIdx.x;
    const int m = COST ? s.m - 1 : s.m;   // (the cost path passes the view with m + 1 rows above the last)
    const int xcol = COST ? n : n + 1;
    double* row = s.T + (size_t)i * s.ld;
    const double* cr = i == m ? c : dir;
    for (int j = threadIdx.x; j < s.ld; j += blockDim.x) {
        double v = 0.0;
        if (i < m) {
            if (j < n) {
                const double a = A[(size_t)j * m + i];
                v = up[j] ? -a : a;
            } else if (!COST && j == n) {
                v = dir[i];
            } else if (j == xcol) {
                v = bp[i];
            }
        } else if (j < n) {
            v = up[j] ? -cr[j] : cr[j];
        }
        row[j] = v;
    }
}

// One block: the basis and the non-basic marks (the RHS path's d column barred), and step 3's test: the basic
// columns as loaded are the unit vectors in order and every cost row is zero there
__global__ __launch_bounds__(1024) void k_bparl_identity(SimplexDev s, int n, const double* A, const double* c,
                                                         const double* g, const int* up, const int* basis,
                                                         BparlRun* run) {
    const int m = s.m, tid = threadIdx.x;
    for (int j = tid; j < s.n; j += blockDim.x) s.nonbasic[j] = j < n ? 1 : 0;
    __syncthreads();
    int bad = 0;
    for (int t = tid; t < m; t += blockDim.x) {
        const int q = basis[t];
        s.basis[t] = q;
        s.nonbasic[q] = 0;
        if (c[q] != 0.0 || (g && g[q] != 0.0)) bad = 1;
    }
    for (size_t e = tid; e < (size_t)m * m && !bad; e += blockDim.x) {
        const int t = (int)(e / m), i = (int)(e - (size_t)t * m);
        const double a = A[(size_t)basis[t] * m + i];
        if ((up[basis[t]] ? -a : a) != ((i == t) ? 1.0 : 0.0)) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) run->identity = !bad;
}

// The cost path's crash: the g' row's eta entry of the step k_crash_select has just staged (one thread)
__global__ void k_bparl_second_eta(SimplexDev s) {
    const SimplexState* st = s.state;
    if (!st->pivot_valid) return;
    const size_t ld = s.ld;
    const double ur = s.T[(size_t)st->leave * ld + st->enter];
    s.lcol[s.m + 1] = -s.T[(size_t)(s.m + 1) * ld + st->enter] / ur;
}

// One block: step 4 and the state word (kRunning, or LP_BAD_ARG for a start that is not optimal at t = 0)
template <bool MX>
__global__ __launch_bounds__(1024) void k_bparl_begin(SimplexDev s, BoundedLargeDev bd, int n, int xcol, double eps,
                                                      BparlRun* run) {
    const int tid = threadIdx.x, m = s.m, ld = s.ld;
    int pinf = 0, dinf = 0;
    for (int t = tid; t < m; t += blockDim.x) {
        const double xb = s.T[(size_t)t * ld + xcol], u = bd.U[s.basis[t]];
        if (xb < -eps || (u < INFINITY && u - xb < -eps)) pinf = 1;
    }
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
        run->tend = 0.0;
        run->k = 0;
    }
}

// ---- the chains of R3 / C3

// Position t's operands at tt: step 5's value of variable k held at tableau value v, the cost entry and the slope
// operand.  be = beta_t (xB_t), de = delta_t (RHS path only).
template <bool COST>
__device__ __forceinline__ void bparl_position(const BoundedLargeDev& bd, const BparlDev& o, int k, double tt,
                                               double be, double de, const BparlLds& L, int t) {
    const double u = bd.U[k], l = o.lo[k];
    const int f = bd.up[k];
    const double v = COST ? be : fma(tt, de, be);
    const double w = f ? u - v : v;
    L.xa[t] = l == 0.0 ? w : l + w;
    if (COST) {
        const double gk = o.g[k];
        L.ca[t] = fma(tt, gk, o.c[k]);
        L.sa[t] = gk;
    } else {
        L.ca[t] = o.c[k];
        L.sa[t] = f ? -de : de;
    }
}

// The two chains on one whole wave (every lane carries the same z and sl): the positions from LDS in order, then
// the non-basic columns held at h_j != 0 in index order (the RHS path's slope chain ends with the positions)
template <bool COST>
__device__ __forceinline__ void bparl_chains(const SimplexDev& s, const BoundedLargeDev& bd, const BparlDev& o,
                                             int m, double tt, const BparlLds& L, double& z, double& sl) {
    z = 0.0;
    sl = 0.0;
#pragma unroll 8
    for (int t = 0; t < m; ++t) {
        const double cv = L.ca[t], xv = L.xa[t], sv = L.sa[t];
        z = fma(cv, xv, z);
        sl = COST ? fma(sv, xv, sl) : fma(cv, sv, sl);
    }
    const int lane = threadIdx.x & 63, n = o.n;
    constexpr int Q = 4;   // 64-column tiles in flight together
    for (int j0 = 0; j0 < n; j0 += 64 * Q) {
        double cj[Q], gj[Q], hj[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {   // (every load unconditional, at a clamped index: all of them in flight together)
            const int j = j0 + 64 * q + lane, jc = j < n ? j : n - 1;
            const bool on = s.nonbasic[jc] != 0;
            const int f = bd.up[jc];
            const double hv = o.hi[jc], lv = o.lo[jc];
            cj[q] = o.c[jc];
            gj[q] = COST ? o.g[jc] : 0.0;
            hj[q] = (j < n && on) ? (f ? hv : lv) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            unsigned long long mask = __ballot(hj[q] != 0.0);
            while (mask) {
                const int src = (int)__builtin_ctzll(mask);
                mask &= mask - 1;
                const double h = lpdev::wave_bcast_f64(hj[q], src), cv = lpdev::wave_bcast_f64(cj[q], src);
                if (COST) {
                    const double gv = lpdev::wave_bcast_f64(gj[q], src);
                    z = fma(fma(tt, gv, cv), h, z);
                    sl = fma(gv, h, sl);
                } else {
                    z = fma(cv, h, z);
                }
            }
        }
    }
}

// The chain wave's part of a selector: segment k's record, then the flag
template <bool COST>
__device__ __forceinline__ void bparl_record(const SimplexDev& s, const BoundedLargeDev& bd, const BparlDev& o, int m,
                                             int k, double tk, const BparlLds& L) {
    double z, sl;
    bparl_chains<COST>(s, bd, o, m, tk, L, z, sl);
    if ((threadIdx.x & 63) == 0) {
        o.t[k] = tk;
        o.obj[k] = z;
        o.slope[k] = sl;
    }
    __hip_atomic_store(L.done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Thread 0 before it writes what the chain wave reads.  The chain wave never waits, so this ends.
__device__ __forceinline__ void bparl_meet(const BparlLds& L) {
    while (__hip_atomic_load(L.done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) __builtin_amdgcn_s_sleep(1);
}

// The waves' tau candidates into one (every scan thread; after the gather's barrier)
__device__ __forceinline__ void bparl_tau(const BparlLds& L, double& bv, int& bk) {
    bv = 0.0;
    bk = -1;
    for (int w = 0; w < 16; ++w) take<false>(L.tauv[w], L.taui[w], bv, bk);
}

// The path's end (thread 0): t[k + 1], nseg, the status; obj[k + 1] is k_bparl_finish's
__device__ __forceinline__ void bparl_close(SimplexState* st, const BparlDev& o, int k, double tend, int status) {
    o.t[k + 1] = tend;
    o.run->tend = tend;
    *o.nseg = k + 1;
    st->status = status;
    st->pivot_valid = 0;
}

// ---- RHS path: one breakpoint.  s.n = n + 1 (column n is d), beta in column s.n.
template <bool MX>
__global__ __launch_bounds__(1024) void k_bparl_select_rhs(SimplexDev s, BoundedLargeDev bd, BparlDev o) {
    SimplexState* st = s.state;
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = s.m, n = o.n, ld = s.ld;
    const BparlLds L = bparl_carve(s_dyn, m);
    const double eps = st->eps;
    const int k = o.run->k;
    const double tk = o.run->tk;
    // 1. the chains' operands and the tau candidates (R2), one position per thread and step
    double bv = 0.0;
    int bk = -1;
    for (int t = tid; t < m; t += blockDim.x) {
        const int kk = s.basis[t];
        const double de = s.T[(size_t)t * ld + n], be = s.T[(size_t)t * ld + n + 1];
        bparl_position<false>(bd, o, kk, tk, be, de, L, t);
        if (de < -eps) {
            take<false>(-be / de, t, bv, bk);
        } else if (de > eps) {
            const double u = bd.U[kk];
            if (u < INFINITY) take<false>((u - be) / de, t, bv, bk);
        }
    }
    wave_take<false>(bv, bk);
    if (lane == 0) {
        L.tauv[wave] = bv;
        L.taui[wave] = bk;
    }
    if (tid == 0) *L.done = 0;
    __syncthreads();
    // 2. the chain wave
    if (wave == 15) {
        bparl_record<false>(s, bd, o, m, k, tk, L);
        return;
    }
    // 3. the other waves
    bparl_tau(L, bv, bk);
    const double ts = bv > tk ? bv : tk;
    if (bk < 0 || ts >= o.t_max) {
        if (tid == 0) {
            o.enter[k] = o.leave[k] = o.side[k] = -1;
            bparl_close(st, o, k, o.t_max, LP_OPTIMAL);
        }
        return;
    }
    const int r = bk;
    const double* trow = s.T + (size_t)r * ld;
    const double* drow = s.T + (size_t)m * ld;
    const int old = s.basis[r];   // (every thread reads it and nonbasic[] before the barrier below; thread 0 writes after)
    const bool comp = trow[n] > eps;   // blocked above: row r is read as if complemented
    const double uold = bd.U[old];
    double best;
    auto quotient = [&](int j) {
        const double t = trow[j], a = comp ? -t : t;
        if (!(s.nonbasic[j] != 0 && a < -eps)) return (double)INFINITY;
        return MX ? drow[j] / a : -drow[j] / a;
    };
    const int e = lpdev::block_chain_select<false, true>(n, eps, best, quotient, bd.q, L.sc, kScan);
    const int status = e < 0 ? LP_INFEASIBLE : k == o.max_breaks ? LP_ITER_LIMIT : kRunning;
    if (status != kRunning) {   // the blocking row leaves no trace
        if (tid == 0) {
            o.leave[k] = old;
            o.side[k] = bd.up[old] ^ (comp ? 1 : 0);
            o.enter[k] = -1;
            bparl_close(st, o, k, ts, status);
        }
        return;
    }
    // stage the pivot on (r, e); the complement lives in the staged row alone
    const double ur = comp ? -trow[e] : trow[e];
    for (int i = tid; i <= m; i += kScan) s.lcol[i] = (i == r) ? 1.0 / ur : -s.T[(size_t)i * ld + e] / ur;
    for (int j = tid; j < ld; j += kScan) {
        double v = trow[j];
        if (comp) v = (j < s.n) ? -v : (j == s.n) ? uold - v : v;
        if (j == old) v = 1.0;   // the leaving variable's own column: the unit column again (a no-op without comp)
        s.prow[j] = v;
    }
    __syncthreads();
    if (tid == 0) {
        bparl_meet(L);
        o.leave[k] = old;
        o.side[k] = bd.up[old] ^ (comp ? 1 : 0);
        o.enter[k] = e;
        if (comp) bd.up[old] ^= 1;
        s.basis[r] = e;
        s.nonbasic[e] = 0;
        s.nonbasic[old] = 1;
        st->iters += 1;
        st->enter = e;
        st->leave = r;
        st->pivot_valid = 1;
        o.run->tk = ts;
        o.run->k = k + 1;
    }
}

// ---- cost path: one breakpoint.  s.m = m (the selector's view); the tableau has rows m (c') and m + 1 (g').
template <bool MX>
__global__ __launch_bounds__(1024) void k_bparl_select_cost(SimplexDev s, BoundedLargeDev bd, BparlDev o) {
    SimplexState* st = s.state;
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (st->status != kRunning) {
        if (tid == 0) st->pivot_valid = 0;
        return;
    }
    const int m = s.m, n = o.n, ld = s.ld;
    double* s_u = s_dyn;                    // m + 2: column e over rows 0..m+1
    double* s_ratio = s_dyn + (m + 2);      // m (+ 2 of padding)
    const BparlLds L = bparl_carve(s_dyn + 2 * (m + 2), m);
    const double eps = st->eps;
    const int k = o.run->k;
    const double tk = o.run->tk;
    // 1. the chains' operands, and the tau candidates over the non-basic columns in index order (C2)
    for (int t = tid; t < m; t += blockDim.x)
        bparl_position<true>(bd, o, s.basis[t], tk, s.T[(size_t)t * ld + n], 0.0, L, t);
    const double* drow = s.T + (size_t)m * ld;
    const double* grow = s.T + (size_t)(m + 1) * ld;
    double bv = 0.0;
    int bk = -1;
    for (int j = tid; j < n; j += blockDim.x) {
        const double dl = grow[j];
        if (s.nonbasic[j] && (MX ? (dl > eps) : (dl < -eps))) take<false>(-drow[j] / dl, j, bv, bk);
    }
    wave_take<false>(bv, bk);
    if (lane == 0) {
        L.tauv[wave] = bv;
        L.taui[wave] = bk;
    }
    if (tid == 0) *L.done = 0;
    __syncthreads();
    // 2. the chain wave
    if (wave == 15) {
        bparl_record<true>(s, bd, o, m, k, tk, L);
        return;
    }
    // 3. the other waves
    bparl_tau(L, bv, bk);
    const double ts = bv > tk ? bv : tk;
    if (bk < 0 || ts >= o.t_max) {
        if (tid == 0) {
            o.enter[k] = o.leave[k] = o.side[k] = -1;
            bparl_close(st, o, k, o.t_max, LP_OPTIMAL);
        }
        return;
    }
    const int e = bk;
    // the bounded ratio test over column e (k_simplex_select_bounded's arithmetic), the chain on the scan threads
    for (int i = m + tid; i <= m + 1; i += kScan) s_u[i] = s.T[(size_t)i * ld + e];
    double theta;
    auto ratio = [&](int i) {
        const double a = s.T[(size_t)i * ld + e], xb = s.T[(size_t)i * ld + n], u = bd.U[s.basis[i]];
        s_u[i] = a;
        return (a > eps) ? xb / a : (a < -eps && u < INFINITY) ? (xb - u) / a : (double)INFINITY;
    };
    const int r = lpdev::block_chain_select<false, true>(m, eps, theta, ratio, s_ratio, L.sc, kScan);
    const double ue = bd.U[e];
    const int status = (r < 0 && !(ue < INFINITY)) ? LP_UNBOUNDED : k == o.max_breaks ? LP_ITER_LIMIT : kRunning;
    if (status != kRunning) {   // the blocking column leaves no trace
        if (tid == 0) {
            o.enter[k] = e;
            o.leave[k] = o.side[k] = -1;
            bparl_close(st, o, k, ts, status);
        }
        return;
    }
    if (r < 0 || ue <= theta) {   // bound flip over rows 0..m+1: e goes to its other bound, the basis stays
        for (int i = tid; i <= m + 1; i += kScan) {
            const size_t row = (size_t)i * ld;
            s.T[row + n] = fma(-ue, s_u[i], s.T[row + n]);
            s.T[row + e] = -s_u[i];
        }
        if (tid == 0) {
            bparl_meet(L);
            const int f = bd.up[e] ^ 1;
            bd.up[e] = f;
            o.enter[k] = e;
            o.leave[k] = e;
            o.side[k] = f;
            st->iters += 1;
            st->pivot_valid = 0;
            o.run->tk = ts;
            o.run->k = k + 1;
        }
        return;
    }
    // pivot on row r over rows 0..m+1; a_r < -eps: the leaving variable stops at its upper bound, complemented first
    const int old = s.basis[r];   // (every thread reads it before the barrier below; thread 0 writes it after)
    const bool comp = s_u[r] < -eps;
    const double ur = comp ? -s_u[r] : s_u[r];
    for (int i = tid; i <= m + 1; i += kScan) s.lcol[i] = (i == r) ? 1.0 / ur : -s_u[i] / ur;
    const double* trow = s.T + (size_t)r * ld;
    const double uold = bd.U[old];
    for (int j = tid; j < ld; j += kScan) {
        double v = trow[j];
        if (comp) v = (j < n) ? -v : (j == n) ? uold - v : v;
        if (j == old) v = 1.0;   // the leaving variable's own column: the unit column again (a no-op without comp)
        s.prow[j] = v;
    }
    __syncthreads();
    if (tid == 0) {
        bparl_meet(L);
        const int f = bd.up[old] ^ (comp ? 1 : 0);
        bd.up[old] = f;
        o.enter[k] = e;
        o.leave[k] = old;
        o.side[k] = f;
        s.basis[r] = e;
        s.nonbasic[e] = 0;
        s.nonbasic[old] = 1;
        st->iters += 1;
        st->enter = e;
        st->leave = r;
        st->pivot_valid = 1;
        o.run->tk = ts;
        o.run->k = k + 1;
    }
}

// obj[nseg] (parametric_ref.c step 4): the value chain at the path's end with the last basis; an end at +inf gives
// obj[nseg - 1] when the last slope is zero, else +inf or -inf by its sign.  One block, after the walk.
template <bool COST>
__global__ __launch_bounds__(1024) void k_bparl_finish(SimplexDev s, BoundedLargeDev bd, BparlDev o) {
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    const int tid = threadIdx.x, m = s.m, n = o.n, ld = s.ld;
    const int k = *o.nseg - 1;
    const double tend = o.run->tend;
    if (tend == INFINITY) {
        if (tid == 0) {
            const double sk = o.slope[k];
            o.obj[k + 1] = sk == 0.0 ? o.obj[k] : sk > 0.0 ? INFINITY : -INFINITY;
        }
        return;
    }
    const BparlLds L = bparl_carve(s_dyn, m);
    for (int t = tid; t < m; t += blockDim.x) {
        const size_t row = (size_t)t * ld;
        if (COST) bparl_position<true>(bd, o, s.basis[t], tend, s.T[row + n], 0.0, L, t);
        else bparl_position<false>(bd, o, s.basis[t], tend, s.T[row + n + 1], s.T[row + n], L, t);
    }
    __syncthreads();
    if (tid < 64) {
        double z, sl;
        bparl_chains<COST>(s, bd, o, m, tend, L, z, sl);
        if (tid == 0) o.obj[k + 1] = z;
    }
}

template <bool COST>
void bparl_launch_select(hipStream_t st, bool maximize, size_t shm, const SimplexDev& s, const BoundedLargeDev& bd,
                         const BparlDev& o) {
    if (COST) {
        if (maximize) hipLaunchKernelGGL(k_bparl_select_cost<true>, 1, 1024, shm, st, s, bd, o);
        else hipLaunchKernelGGL(k_bparl_select_cost<false>, 1, 1024, shm, st, s, bd, o);
    } else {
        if (maximize) hipLaunchKernelGGL(k_bparl_select_rhs<true>, 1, 1024, shm, st, s, bd, o);
        else hipLaunchKernelGGL(k_bparl_select_rhs<false>, 1, 1024, shm, st, s, bd, o);
    }
}

template <bool COST>
int bparl_run(lp_context* ctx, const BasisBoundedParametricDev& d, int* nseg_host) {
    hipStream_t st = ctx->stream;
    const int m = d.m, n = d.n, maximize = d.maximize;
    const int cols = COST ? n : n + 1;   // tableau columns left of the right-hand side
    const int rows = COST ? m + 2 : m + 1;
    const int ld = (int)lp_ceil_div<size_t>((size_t)cols + 1, 8) * 8;
    const size_t row_bytes = sizeof(double) * (size_t)ld;
    const size_t shm = bparl_lds_bytes(m, COST), shm_finish = bparl_lds_bytes(m, false);
    const void* selector = COST ? (maximize ? reinterpret_cast<const void*>(k_bparl_select_cost<true>)
                                            : reinterpret_cast<const void*>(k_bparl_select_cost<false>))
                                : (maximize ? reinterpret_cast<const void*>(k_bparl_select_rhs<true>)
                                            : reinterpret_cast<const void*>(k_bparl_select_rhs<false>));
    LP_HIP(ctx, lp_lds_opt_in(selector, shm));
    LP_HIP(ctx, lp_lds_opt_in(reinterpret_cast<const void*>(k_bparl_finish<COST>), shm_finish));

    lp_simplex_problem q;   // the crash's and the selectors' view: m constraint rows, the cost row m
    q.ctx = ctx;
    q.tableau_bytes = row_bytes * (size_t)(m + 1);
    SimplexDev& sd = q.dev;
    sd.m = m;
    sd.n = cols;
    sd.ld = ld;
    sd.maximize = maximize ? 1 : 0;
    // one allocation: T, the crash's permutation buffer (rows 0..m), lcol, prow, state, basis, rowpos, rowused,
    // nonbasic; the bound state; b' and the run record
    BoundedLargeDev bd{};
    double* bp;
    BparlRun* run;
    auto pieces = [&](lp_carver& cv) {
        sd.T = cv.take<double>(row_bytes * (size_t)rows);
        q.dT0 = cv.take<double>(q.tableau_bytes);
        sd.lcol = cv.take<double>(sizeof(double) * (size_t)rows);
        sd.prow = cv.take<double>(row_bytes);
        sd.state = cv.take<SimplexState>(sizeof(SimplexState));
        sd.basis = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowpos = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowused = cv.take<unsigned char>((size_t)m);
        sd.nonbasic = cv.take<unsigned char>((size_t)cols);
        bd.U = cv.take<double>(sizeof(double) * (size_t)cols);
        bd.q = cv.take<double>(row_bytes);
        bd.up = cv.take<int>(sizeof(int) * (size_t)cols);
        bd.flips = cv.take<int>(sizeof(int));
        bp = cv.take<double>(sizeof(double) * (size_t)m);
        run = cv.take<BparlRun>(sizeof(BparlRun));
    };
    lp_device_buffer arena;
    LP_HIP(ctx, lp_carve_malloc(&arena.ptr, pieces));
    lp_simplex_problem qv;   // the update's view on the cost path: rows 0..m+1
    qv.ctx = ctx;
    qv.dev = sd;
    if (COST) qv.dev.m = m + 1;
    const BparlDev o{n, d.max_breaks, d.t_max, d.c, COST ? d.dir : nullptr, d.lo, d.hi, d.nseg, d.t, d.obj, d.slope,
                     d.enter, d.leave, d.side, run};
    SimplexState* hstate = nullptr;
    LP_HIP(ctx, hipHostMalloc(&hstate, sizeof(SimplexState)));
    struct Pinned {
        SimplexState* p;
        ~Pinned() { (void)hipHostFree(p); }
    } pinned{hstate};
    q.h_state = hstate;
    *nseg_host = 0;

    LP_HIP(ctx, hipMemsetAsync(d.nseg, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_bparl_bounds, lp_ceil_div(cols, 256), 256, 0, st, n, cols, d.lo, d.hi, d.at_upper, bd.U, bd.up);
    hipLaunchKernelGGL(k_bparl_bprime, lp_ceil_div(m, 64), 64, 0, st, d.A, m, n, d.b, d.lo, bd.U, bd.up, bp);
    hipLaunchKernelGGL(k_bparl_gather<COST>, rows, 256, 0, st, qv.dev, n, d.A, bp, d.c, d.dir, bd.up);
    hipLaunchKernelGGL(k_bparl_identity, 1, 1024, 0, st, sd, n, d.A, d.c, COST ? d.dir : nullptr, bd.up, d.basis, run);
    BparlRun hr{};
    LP_HIP(ctx, hipMemcpyAsync(&hr, run, sizeof(hr), hipMemcpyDeviceToHost, st));
    LP_HIP(ctx, hipStreamSynchronize(st));
    LP_HIP(ctx, hipGetLastError());
    int rc = LP_OPTIMAL;
    if (!hr.identity) {
        if (COST) rc = lp_simplex_crash(&q, &qv, [&] { hipLaunchKernelGGL(k_bparl_second_eta, 1, 1, 0, st, sd); });
        else rc = lp_simplex_crash(&q);
    }
    if (rc != LP_OPTIMAL) return rc;   // LP_SINGULAR, or a HIP error
    if (maximize)
        hipLaunchKernelGGL(k_bparl_begin<true>, 1, 1024, 0, st, sd, bd, n, COST ? n : n + 1, d.eps, run);
    else
        hipLaunchKernelGGL(k_bparl_begin<false>, 1, 1024, 0, st, sd, bd, n, COST ? n : n + 1, d.eps, run);
    rc = lp_poll_pivots(&q, [&](int batch) {
        for (int k = 0; k < batch; ++k) {
            bparl_launch_select<COST>(st, maximize != 0, shm, sd, bd, o);
            lp_simplex_launch_update(&qv);
        }
        return 2 * batch;
    });
    if (rc != LP_OPTIMAL) return rc;
    rc = hstate->status;
    if (rc == LP_BAD_ARG) return rc;   // the start is not optimal: no path
    hipLaunchKernelGGL(k_bparl_finish<COST>, 1, 1024, shm_finish, st, sd, bd, o);
    LP_HIP(ctx, hipMemcpyAsync(d.basis_out, sd.basis, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, st));
    LP_HIP(ctx, hipMemcpyAsync(d.at_upper_out, bd.up, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st));
    LP_HIP(ctx, hipMemcpyAsync(nseg_host, d.nseg, sizeof(int), hipMemcpyDeviceToHost, st));
    LP_HIP(ctx, hipStreamSynchronize(st));
    LP_HIP(ctx, hipGetLastError());
    return rc;
}

}  // namespace

size_t lp_basis_bounded_parametric_large_lds_bytes(int m, bool cost) { return bparl_lds_bytes(m, cost); }

int lp_basis_bounded_parametric_device(lp_context* ctx, const BasisBoundedParametricDev& d, bool cost,
                                       int* nseg_host) {
    if (lp_basis_bounded_parametric_large_lds_bytes(d.m, cost) > 156 * 1024)
        LP_FAIL(ctx, LP_BAD_ARG, "bounded basis parametric: m too large for the selector's LDS");
    return cost ? bparl_run<true>(ctx, d, nseg_host) : bparl_run<false>(ctx, d, nseg_host);
}
