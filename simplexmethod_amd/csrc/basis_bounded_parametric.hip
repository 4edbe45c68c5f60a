// basis_bounded_parametric.hip — the parametric right-hand-side path z*(t) = opt { c.x : A x = b + t d, lo <= x <= hi }
// and the parametric cost path z*(t) = opt { (c + t g).x : A x = b, lo <= x <= hi } of a bounded-variable LP from a
// given optimal basis and its at-upper flags, for t from 0 up to t_max, exactly as tests/ref/bounded_parametric_ref.c
// states them (the step numbers below are its):
//   - the tableau of batched_bounded_resolve.hip (shifted variables, every flagged column held complemented, b' one
//     serial fma chain per row) with one more right-hand column (RHS path: slot n holds b', slot n+1 holds d, which is
//     neither shifted nor complemented) or one more cost row (cost path: row m holds c', row m+1 holds g', both negated
//     in the flagged columns); the basis installed by batched_resolve_crash.hpp over every stored row and column;
//   - start check: no position violated below or above and no dual infeasibility at t = 0, else LP_BAD_ARG;
//   - RHS segment (R2): tau_t = -beta_t / delta_t for delta_t < -eps, (U - beta_t) / delta_t for delta_t > eps with a
//     finite U; the first strict minimum (basis_crash.hpp's take); blocked above, row r is read complemented by the
//     dual entering chain (batched_bounded_dual_loop.hpp's), and the complement is applied only when the pivot is;
//   - cost segment (C2): tau_s = -d_s / delta_s over the slots of a variable < n, keyed by variable; then the bounded
//     ratio test of batched_bounded_loop.hpp with its three outcomes: unbounded, bound flip (rows 0..m+1), pivot with
//     the leaving variable complemented first when it stops at its upper bound;
//   - values (R3 / C3) in the caller's variables: the chain over the positions continued over the held non-basic
//     columns, and the slope chain, serial by definition: they run on lane 0 of wave 1 while wave 0 selects.
//
// k_batched_bounded_parametric<NT, MX> and k_batched_bounded_parametric_cost<NT, MX>: one LP per workgroup, all state
// in LDS.  Both are bounded_parametric_body<NT, MX, COST>; the carve is batched_bounded_carve.hpp's for one more column
// (m, n + 1) or one more row (m + 1, n), followed by hi, c, g and the held values of the non-basic columns (n doubles
// each), the end of the segment (one double), the slot of every variable (n ints) and one more published word.  The
// sense is a template parameter (with a run-time flag selecting the comparison, -O3 reductions returned
// wrong winners on gfx950).  The pivot is
// batched_lds_loop.hpp's over `rows` rows (that file's stops at row m), as in basis_parametric_cost.hip.  Every loop
// exit is decided by a word published before a barrier or by block_any.  There is no path beyond
// lp_basis_bounded_parametric_fits / _cost_fits, as in the bounded family.
#include <cfloat>
#include <climits>

#include "basis_crash.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"
#include "batched_bounded_carve.hpp"
#include "device_select.hpp"
#include "lp_internal.hpp"

namespace {

enum { kGoOn = 0, kEndTMax = 1, kEndInfeasible = 2, kEndUnbounded = 3, kEndLimit = 4 };
enum { kActPivot = 0, kActFlip = 1, kActComplement = 2 };   // the cost path's pub2[0]; the RHS path's: blocked above

__host__ __device__ inline int bpar_status(int code) {
    return code == kEndInfeasible ? LP_INFEASIBLE
           : code == kEndUnbounded ? LP_UNBOUNDED
           : code == kEndLimit     ? LP_ITER_LIMIT
                                   : LP_OPTIMAL;
}

// The bounded carve for one more column or row, then this file's own pieces (byte offsets, alike on host and device)
struct BparCarve {
    BoundedCarve K;
    size_t tend, hiv, cv, gv, hval, varslot, pub2, bytes;
};

__host__ __device__ inline BparCarve bpar_carve(int m, int n, bool cost) {
    BparCarve q{};
    q.K = cost ? bounded_carve(m + 1, n) : bounded_carve(m, n + 1);
    size_t o = q.K.bytes;
    q.tend = o;
    o += sizeof(double) * 2;
    q.hiv = o;
    o += sizeof(double) * (size_t)n;
    q.cv = o;
    o += sizeof(double) * (size_t)n;
    q.gv = o;
    o += cost ? sizeof(double) * (size_t)n : 0;
    q.hval = o;
    o += sizeof(double) * (size_t)n;
    q.varslot = o;
    o += sizeof(int) * (size_t)n;
    q.pub2 = o;
    o += sizeof(int) * 4;
    q.bytes = (o + 15) & ~(size_t)15;
    return q;
}

template <int NT, bool MX, bool COST>
__device__ __forceinline__ void bounded_parametric_body(const BasisBoundedParametricDev& d, double* smem) {
    char* base = reinterpret_cast<char*>(smem);
    const int m = d.m, n = d.n;
    const int rows = COST ? m + 2 : m + 1;   // stored rows: the cost row(s) last
    const int W = COST ? n + 1 : n + 2;      // stored columns: the right-hand column(s) last
    const BparCarve Q = bpar_carve(m, n, COST);
    const int pitch = Q.K.pitch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = reinterpret_cast<double*>(base + Q.K.T);
    double* prow = reinterpret_cast<double*>(base + Q.K.prow);
    double* lcol = reinterpret_cast<double*>(base + Q.K.lcol);
    double* U = reinterpret_cast<double*>(base + Q.K.U);
    double* lov = reinterpret_cast<double*>(base + Q.K.lov);
    int* slotvar = reinterpret_cast<int*>(base + Q.K.slotvar);
    int* basis = reinterpret_cast<int*>(base + Q.K.basis);
    int* up = reinterpret_cast<int*>(base + Q.K.up);
    double* pend = reinterpret_cast<double*>(base + Q.tend);   // [0] the end of the segment wave 0 has just closed
    double* hiv = reinterpret_cast<double*>(base + Q.hiv);
    double* cv = reinterpret_cast<double*>(base + Q.cv);
    double* gv = reinterpret_cast<double*>(base + Q.gv);       // (cost path only)
    double* hval = reinterpret_cast<double*>(base + Q.hval);   // the held value of a non-basic column, 0.0 if basic
    int* varslot = reinterpret_cast<int*>(base + Q.varslot);   // slot of a non-basic variable < n, -1 if basic
    int* pub2 = reinterpret_cast<int*>(base + Q.pub2);         // [0] blocked above (RHS) / the action (cost)
    int* pub = pubs->v;   // [0] entering slot / crash row, [1] leaving position, [2] verdict / end code, [3] block_any

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* lo = d.lo + (size_t)lp * n;
    const double* hi = d.hi + (size_t)lp * n;
    const double* dir = d.dir + (size_t)lp * (COST ? n : m);
    const int* N = d.basis + (size_t)lp * m;
    const int* upin = d.at_upper + (size_t)lp * n;
    const double eps = d.eps;
    const int MB = d.max_breaks;
    double* t_out = d.t + (size_t)lp * (MB + 2);
    double* obj_out = d.obj + (size_t)lp * (MB + 2);
    double* slope_out = d.slope + (size_t)lp * (MB + 1);
    int* enter_out = d.enter + (size_t)lp * (MB + 1);
    int* leave_out = d.leave + (size_t)lp * (MB + 1);
    int* side_out = d.side + (size_t)lp * (MB + 1);
    constexpr int ANY_WORD = 3;   // block_any's word of pub
#include "batched_block_any.hpp"

    // step 5: the caller's value of variable k held at tableau value v
    auto xval = [&](int k, double v) {
        const double w = up[k] ? U[k] - v : v;
        const double l = lov[k];
        return l == 0.0 ? w : l + w;
    };
    // R3 / C3 on one lane: the value chain at tt and the slope chain, over the positions and then over the held
    // non-basic columns
    auto chains = [&](double tt, double& z, double& sl) {
        z = 0.0;
        sl = 0.0;
        for (int t = 0; t < m; ++t) {
            const int k = basis[t];
            if (COST) {
                const double x = xval(k, T[(size_t)t * pitch + n]);
                z = fma(fma(tt, gv[k], cv[k]), x, z);
                sl = fma(gv[k], x, sl);
            } else {
                const double de = T[(size_t)t * pitch + n + 1];
                z = fma(cv[k], xval(k, fma(tt, de, T[(size_t)t * pitch + n])), z);
                sl = fma(cv[k], up[k] ? -de : de, sl);
            }
        }
        // (a term with h == 0.0 is skipped, which covers the basic columns; as selects, so that the loads of the next
        // columns do not wait for the chain)
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const double h = hval[j];
            if (COST) {
                const double zj = fma(fma(tt, gv[j], cv[j]), h, z), sj = fma(gv[j], h, sl);
                z = h != 0.0 ? zj : z;
                sl = h != 0.0 ? sj : sl;
            } else {
                const double zj = fma(cv[j], h, z);
                z = h != 0.0 ? zj : z;
            }
        }
    };

    const int run = d.run_status ? d.run_status[lp] : LP_OPTIMAL;
    int status = run;
    int nseg = 0;
    if (status == LP_OPTIMAL) {
        // ---- load (batched_bounded_resolve.hip's): slots = the columns in order, a flagged one sign-changed in every
        // row; basis = the artificials by row
        int bad = 0;
        for (int s = tid; s < n; s += NT) {
            const double l = lo[s], h = hi[s], u = h - l;
            const int f = upin[s];
            slotvar[s] = s;
            up[s] = f;
            lov[s] = l;
            hiv[s] = h;
            U[s] = u;
            cv[s] = c[s];
            T[(size_t)m * pitch + s] = f ? -c[s] : c[s];
            if (COST) {
                gv[s] = dir[s];
                T[(size_t)(m + 1) * pitch + s] = f ? -dir[s] : dir[s];
            }
            if (u < 0.0) bad = 1;
        }
        for (int e = tid; e < (rows - m) * (W - n); e += NT)   // the right-hand entries of the cost row(s)
            T[(size_t)(m + e / (W - n)) * pitch + n + e % (W - n)] = 0.0;
        for (int t = tid; t < m; t += NT) basis[t] = n + t;
        for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
            const int s = e / m, i = e - s * m;
            const double a = A[e];
            T[(size_t)i * pitch + s] = upin[s] ? -a : a;
        }
        if (block_any(bad)) status = LP_INFEASIBLE;   // crossed bounds
    }
    if (status == LP_OPTIMAL) {
        // ---- b' (one chain per row): the shift over lo_j != 0, then the complements over the flagged columns
        for (int i = tid; i < m; i += NT) {
            const double* row = T + (size_t)i * pitch;
            double acc = b[i];
            for (int j = 0; j < n; ++j) {
                const double l = lov[j];
                if (l != 0.0) acc = fma(up[j] ? row[j] : -row[j], l, acc);   // (-A_ij: a flagged slot holds it)
            }
            for (int j = 0; j < n; ++j)
                if (up[j]) acc = fma(row[j], U[j], acc);
            T[(size_t)i * pitch + n] = acc;
            if (!COST) T[(size_t)i * pitch + n + 1] = dir[i];
        }
        // the crash is skipped when the basic columns, as loaded, are the unit vectors in order with zero costs
        int not_identity = 0;
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m;
            if (T[(size_t)i * pitch + N[t]] != ((i == t) ? 1.0 : 0.0)) not_identity = 1;
        }
        for (int t = tid; t < m; t += NT) {
            if (T[(size_t)m * pitch + N[t]] != 0.0) not_identity = 1;
            if (COST && T[(size_t)(m + 1) * pitch + N[t]] != 0.0) not_identity = 1;
        }
        const bool identity = !block_any(not_identity);

        // ---- one Gauss-Jordan pivot on (row r, slot se) over all stored rows and columns with tableau_pivot's
        // arithmetic (batched_lds_loop.hpp's); slot se receives the leaving variable's column.  All threads.
        const int G = NT / W > 0 ? NT / W : 1;   // row groups: a thread owns one column and every G-th row
        auto pivot = [&](int r, int se) {
            const double ur = T[(size_t)r * pitch + se];
            for (int j = tid; j < W; j += NT) prow[j] = T[(size_t)r * pitch + j];
            for (int i = tid; i < rows; i += NT) lcol[i] = (i == r) ? 1.0 / ur : -T[(size_t)i * pitch + se] / ur;
            __syncthreads();
            for (int slot = tid; slot < G * W; slot += NT) {
                const int j = slot % W, gr = slot / W;
                const double pj = prow[j];
                for (int i = gr; i < rows; i += G) {
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
        // the complement of batched_bounded_loop.hpp / batched_bounded_dual_loop.hpp: row r's n slots negated,
        // xB_r = U_r - xB_r (the RHS path: delta_r negated too), the flag toggled
        auto complement = [&](int r) {
            const int k = basis[r];
            for (int j = tid; j < n; j += NT) T[(size_t)r * pitch + j] = -T[(size_t)r * pitch + j];
            if (tid == 0) {
                T[(size_t)r * pitch + n] = U[k] - T[(size_t)r * pitch + n];
                if (!COST) T[(size_t)r * pitch + n + 1] = -T[(size_t)r * pitch + n + 1];
                up[k] ^= 1;
            }
            __syncthreads();
        };
#include "batched_resolve_crash.hpp"

        const double* drow = T + (size_t)m * pitch;
        if (status == LP_OPTIMAL) {
            // ---- the slot of every variable, and the start check (batched_bounded_resolve.hip's classification)
            for (int j = tid; j < n; j += NT) varslot[j] = -1;
            __syncthreads();
            int pinf = 0, dinf = 0;
            for (int s = tid; s < n; s += NT) {
                const int k = slotvar[s];
                if (k < n) {
                    varslot[k] = s;
                    if (MX ? (drow[s] > eps) : (drow[s] < -eps)) dinf = 1;
                }
            }
            for (int t = tid; t < m; t += NT) {
                const double xb = T[(size_t)t * pitch + n], u = U[basis[t]];
                if (xb < -eps || (u < INFINITY && u - xb < -eps)) pinf = 1;
            }
            const bool violated = block_any(pinf);
            const bool dual_infeasible = block_any(dinf);
            if (violated || dual_infeasible) status = LP_BAD_ARG;
            for (int j = tid; j < n; j += NT) hval[j] = varslot[j] < 0 ? 0.0 : up[j] ? hiv[j] : lov[j];
            __syncthreads();
        }
        if (status == LP_OPTIMAL) {
            // ---- the segments.  Lane 0 of wave 1 (tid 64) writes t, obj and slope of segment k while wave 0 selects
            // and writes enter, leave and side; tk is the same in every thread (pend[0] after the barrier)
            double tk = 0.0, zk = 0.0, sk = 0.0;
            int k = 0, code = kGoOn;
            for (;; ++k) {
                if (tid == 64) {
                    chains(tk, zk, sk);
                    t_out[k] = tk;
                    obj_out[k] = zk;
                    slope_out[k] = sk;
                }
                if (wave == 0) {
                    double bv = 0.0;
                    int bk = -1;
                    if (COST) {   // tau over the slots of a variable < n, keyed by variable
                        const double* grow = T + (size_t)(m + 1) * pitch;
                        for (int s = lane; s < n; s += 64) {
                            const int v = slotvar[s];
                            const double dl = grow[s];
                            if (v < n && (MX ? (dl > eps) : (dl < -eps))) take<false>(-drow[s] / dl, v, bv, bk);
                        }
                    } else {      // tau over the positions: t ascending per lane, take keeps the first minimum
                        for (int t = lane; t < m; t += 64) {
                            const double de = T[(size_t)t * pitch + n + 1], be = T[(size_t)t * pitch + n];
                            if (de < -eps) {
                                take<false>(-be / de, t, bv, bk);
                            } else if (de > eps) {
                                const double u = U[basis[t]];
                                if (u < INFINITY) take<false>((u - be) / de, t, bv, bk);
                            }
                        }
                    }
                    wave_take<false>(bv, bk);
                    const double ts = bv > tk ? bv : tk;
                    int se0 = -1, r0 = -1, cd = kGoOn, act = 0;
                    double tend = ts;
                    if (bk < 0 || ts >= d.t_max) {
                        cd = kEndTMax;
                        tend = d.t_max;
                        if (lane == 0) enter_out[k] = leave_out[k] = side_out[k] = -1;
                    } else if (!COST) {
                        // blocked above: the dual entering chain reads row r as if complemented
                        r0 = bk;
                        const double* rrow = T + (size_t)r0 * pitch;
                        act = rrow[n + 1] > eps;
                        double best;
                        se0 = wave_scan_keyed<false>(n, eps, best, [&](int s, double& v, int& key, bool& ok) {
                            const double a = act ? -rrow[s] : rrow[s];
                            key = slotvar[s];
                            ok = key < n && a < -eps;
                            v = MX ? drow[s] / a : -drow[s] / a;
                        });
                        cd = se0 < 0 ? kEndInfeasible : k == MB ? kEndLimit : kGoOn;
                        if (lane == 0) {
                            const int kl = basis[r0];
                            leave_out[k] = kl;
                            side_out[k] = up[kl] ^ act;
                            enter_out[k] = cd == kGoOn ? slotvar[se0] : -1;
                        }
                    } else {
                        // batched_bounded_loop.hpp's ratio test over the slot of column bk, code for code
                        const int se = varslot[bk];
                        se0 = se;
                        auto ratio = [&](int i) -> double {
                            const double a = T[(size_t)i * pitch + se], xb = T[(size_t)i * pitch + n];
                            const double u = U[basis[i]];
                            return (a > eps) ? xb / a : (a < -eps && u < INFINITY) ? (xb - u) / a : INFINITY;
                        };
                        if (m <= 128) {
                            double rv[2];
#pragma unroll
                            for (int q = 0; q < 2; ++q) {
                                const int i = lane + 64 * q;
                                rv[q] = (i < m) ? ratio(i) : INFINITY;
                            }
                            r0 = wave_ratio_select<2>(rv, m, eps);
                        } else if (m <= 256) {
                            double rv[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int i = lane + 64 * q;
                                rv[q] = (i < m) ? ratio(i) : INFINITY;
                            }
                            r0 = wave_ratio_select<4>(rv, m, eps);
                        } else {
                            double theta;
                            auto getr = [&](int i, double& v, int& key, bool& ok) {
                                v = ratio(i);
                                key = i;
                                ok = true;
                            };
                            r0 = wave_scan_keyed<false>(m, eps, theta, getr);
                        }
                        const double ue = U[bk];
                        if (r0 < 0) act = (ue < INFINITY) ? kActFlip : -1;
                        else if (ue <= ratio(r0)) act = kActFlip;   // (theta: the selected row's value, the same division)
                        else act = (T[(size_t)r0 * pitch + se] < -eps) ? kActComplement : kActPivot;
                        cd = act < 0 ? kEndUnbounded : k == MB ? kEndLimit : kGoOn;
                        if (lane == 0) {
                            enter_out[k] = bk;
                            if (cd != kGoOn) {
                                leave_out[k] = side_out[k] = -1;
                            } else if (act == kActFlip) {
                                leave_out[k] = bk;
                                side_out[k] = up[bk] ^ 1;
                            } else {
                                const int kl = basis[r0];
                                leave_out[k] = kl;
                                side_out[k] = act == kActComplement ? up[kl] ^ 1 : up[kl];
                            }
                        }
                    }
                    if (lane == 0) {
                        pub[0] = se0;
                        pub[1] = r0;
                        pub[2] = cd;
                        pub2[0] = act;
                        pend[0] = tend;
                    }
                }
                __syncthreads();
                const int se = pub[0], r = pub[1], act = pub2[0];
                code = pub[2];
                tk = pend[0];
                if (code != kGoOn) break;
                if (COST && act == kActFlip) {
                    // bound flip: xB (both cost rows' right-hand entries included) moves by U_e times the column,
                    // then the column is negated
                    const int e = slotvar[se];
                    const double ue = U[e];
                    for (int i = tid; i < rows; i += NT) {
                        double* te = T + (size_t)i * pitch + se;
                        double* xb = T + (size_t)i * pitch + n;
                        *xb = fma(-ue, *te, *xb);
                        *te = -*te;
                    }
                    if (tid == 0) {
                        up[e] ^= 1;
                        hval[e] = up[e] ? hiv[e] : lov[e];
                    }
                    __syncthreads();
                    continue;
                }
                if (COST ? act == kActComplement : act != 0) complement(r);
                if (tid == 0) {   // (pivot swaps slotvar[se] and basis[r] after its first barrier)
                    const int ve = slotvar[se], vl = basis[r];
                    varslot[ve] = -1;
                    varslot[vl] = se;
                    hval[ve] = 0.0;
                    hval[vl] = up[vl] ? hiv[vl] : lov[vl];
                }
                pivot(r, se);
            }
            nseg = k + 1;
            status = bpar_status(code);
            if (tid == 64) {   // the last segment's end (tk by now), with the last basis
                double ze, se_;
                t_out[k + 1] = tk;
                if (tk == INFINITY) {
                    ze = sk == 0.0 ? zk : sk > 0.0 ? INFINITY : -INFINITY;
                } else {
                    chains(tk, ze, se_);
                }
                obj_out[k + 1] = ze;
            }
        }
    }
    // ---- outputs past the path: NaN / -1; the final basis and flags (the given ones without a path)
    for (int j = (nseg ? nseg + 1 : 0) + tid; j < MB + 2; j += NT) {
        t_out[j] = NAN;
        obj_out[j] = NAN;
    }
    for (int j = nseg + tid; j < MB + 1; j += NT) {
        slope_out[j] = NAN;
        enter_out[j] = -1;
        leave_out[j] = -1;
        side_out[j] = -1;
    }
    for (int t = tid; t < m; t += NT) d.basis_out[(size_t)lp * m + t] = nseg ? basis[t] : N[t];
    for (int j = tid; j < n; j += NT) d.at_upper_out[(size_t)lp * n + j] = nseg ? up[j] : upin[j];
    if (tid == 0) {
        d.nseg[lp] = nseg;
        d.status[lp] = status;
    }
}

template <int NT, bool MX>
__global__ __launch_bounds__(NT) void k_batched_bounded_parametric(BasisBoundedParametricDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    bounded_parametric_body<NT, MX, false>(d, smem);
}

template <int NT, bool MX>
__global__ __launch_bounds__(NT) void k_batched_bounded_parametric_cost(BasisBoundedParametricDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    bounded_parametric_body<NT, MX, true>(d, smem);
}

}  // namespace

size_t lp_basis_bounded_parametric_lds_bytes(int m, int n, bool cost) { return bpar_carve(m, n, cost).bytes; }

bool lp_basis_bounded_parametric_fits_shape(int m, int n, bool cost) {
    return m > 0 && n >= m && lp_bounded_fits_shape(m, n) &&
           lp_basis_bounded_parametric_lds_bytes(m, n, cost) <= 160 * 1024;
}

int lp_basis_bounded_parametric_launch(lp_context* ctx, const BasisBoundedParametricDev& d, bool cost) {
    if (!lp_basis_bounded_parametric_fits_shape(d.m, d.n, cost))
        LP_FAIL(ctx, LP_BAD_ARG, "bounded basis parametric: the shape does not fit one CU's LDS");
    if (d.batch <= 0) return LP_OPTIMAL;
    const size_t cells = (size_t)(d.m + 1) * (d.n + 1), shm = lp_basis_bounded_parametric_lds_bytes(d.m, d.n, cost);
    if (cost) {
        if (d.maximize)
            return lp_launch_per_lp(ctx, cells, k_batched_bounded_parametric_cost<256, true>,
                                    k_batched_bounded_parametric_cost<1024, true>, shm, d);
        return lp_launch_per_lp(ctx, cells, k_batched_bounded_parametric_cost<256, false>,
                                k_batched_bounded_parametric_cost<1024, false>, shm, d);
    }
    if (d.maximize)
        return lp_launch_per_lp(ctx, cells, k_batched_bounded_parametric<256, true>,
                                k_batched_bounded_parametric<1024, true>, shm, d);
    return lp_launch_per_lp(ctx, cells, k_batched_bounded_parametric<256, false>,
                            k_batched_bounded_parametric<1024, false>, shm, d);
}
