// basis_bounded_certificate.hip — Farkas and unbounded-ray certificates of a bounded-variable LP (A x = b,
// lo <= x <= hi) at a given basis and given at-upper flags, exactly as tests/ref/bounded_certificate_ref.c states them,
// in the caller's original variables:
//   - a non-basic column is held at v_j = hi_j (flagged) or lo_j; the flags of basic columns are not read;
//   - b' = b - sum_j A_j v_j and b0 = b - sum_j A_j lo_j: one fma chain each per row, j ascending, zero terms skipped;
//     a basis index n+i is the artificial of row i, column s_i e_i (s_i = -1 when b0[i] < -eps, else +1);
//   - Binv and xB by ranging's crash on [B | I | b'] (basis_crash.hpp, kept in place in m x (m+1));
//   - the sign test of a weight vector g: every non-basic j has g_j >= -eps at lo_j, g_j <= eps at hi_j;
//   - phase-I case (an artificial is basic): f = -(sum of Binv's artificial rows), FARKAS when the artificials' values
//     sum > eps and g = A^T f passes;
//   - dual-simplex case (no artificial, some xB[t] < L_t - eps or > H_t + eps, H_t finite): the first such t whose
//     alpha row (negated when above) passes, f = +-Binv[t][:]; value = b'^T f - L_t or + H_t;
//   - ray case (otherwise): d_j = c_j - sum_t c_B[t] alpha[t][j] in position order, the first non-basic unflagged j
//     with hi_j = +inf that improves by more than eps with alpha[t][j] <= eps, and >= -eps or H_t = +inf, for every t.
//
// k_batched_bounded_certificate: one LP per workgroup, state in LDS: the structure of k_batched_certificate (the case
// chosen once per workgroup, the alpha chains of basis_col_chains.hpp) plus what k_batched_bounded_sens carries: v (n),
// the basic columns' L and H (2m), b' (m), and in pos the lower / basic / upper code of every column.
//
// Shapes beyond lp_basis_bounded_certificate_fits (lp_basis_bounded_certificate_device, one LP): the column codes, the
// held values, b' and b0 by the small kernels of basis_bounded_kernels.hpp (b0 is the b' chain with lo held);
// k_bcert_gather builds [B | I | b'; 0] with the artificial columns explicit and the single-LP launch pair
// (lp_simplex_crash) pivots it; k_binv_times_a (basis_ranging.hip) forms B^-1 A; then k_bcert_prepare, k_bcert_columns
// and k_bcert_finish choose the case and reduce, as basis_certificate.hip's three do, under the box's rules.
#include <cfloat>

#include "basis_bounded_kernels.hpp"
#include "basis_col_chains.hpp"
#include "basis_crash.hpp"
#include "batched_problem.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kR = 8;   // weight rows per alpha pass

enum { kAtLower = -1, kAtUpper = -2 };   // pos[j] of a non-basic column; a basic column holds its position (>= 0)

__host__ __device__ inline int bcert_threads(int m) { return m <= 64 ? 256 : 512; }
__host__ __device__ inline int bcert_pitch(int m) { return (m + 1) | 1; }
// doubles of the region that holds lcol + prow during the crash, then the A tiles
__host__ __device__ inline size_t bcert_scratch(int m) {
    const size_t tile = (size_t)kCW * (kTR + 1), eta = 2 * (size_t)m + 1;
    return tile > eta ? tile : eta;
}

template <int NT, bool MX>
__global__ __launch_bounds__(NT) void k_batched_bounded_certificate(BasisBoundedCertificateDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int m = d.m, n = d.n, pitch = bcert_pitch(m);
    const int tid = threadIdx.x;
    const int lp = blockIdx.x;
    const double eps = d.eps;
    // ---- LDS carve
    int* pub = reinterpret_cast<int*>(smem);        // [0] pivot row, [1] singular verdict, [2] block_any, [3] pick
    double* T = smem + 2;                           // m x pitch
    double* U = T + (size_t)m * pitch;              // lcol + prow | the A tiles
    double* fv = U + bcert_scratch(m);              // m: the artificials' signs, then f, or the ray's alpha column
    double* bp = fv + m;                            // m: b'
    double* vv = bp + m;                            // n: the held values (0.0 for basic columns)
    double* Lv = vv + n;                            // m: lo of the basic columns by position
    double* Hv = Lv + m;                            // m: hi of the basic columns by position
    int* rowpos = reinterpret_cast<int*>(Hv + m);   // m
    int* used = rowpos + m;                         // m: the crash's flags, then a position list
    int* zneg = used + m;                           // m
    int* slot = zneg + m;                           // m: slot[i] holds identity column m+i
    int* pos = slot + m;                            // n: position of a basic column, kAtLower / kAtUpper otherwise
    int* okr = pos + n;                             // kR
    double* lcol = U;
    double* prow = U + m;

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* lo = d.lo + (size_t)lp * n;
    const double* hi = d.hi + (size_t)lp * n;
    const int* N = d.basis + (size_t)lp * m;
    const int* up = d.at_upper + (size_t)lp * n;
    double* farkas = d.farkas + (size_t)lp * m;
    double* ray = d.ray + (size_t)lp * n;
    constexpr int ANY_WORD = 2;   // block_any's word of pub
#include "batched_block_any.hpp"
    auto binv = [&](int t, int i) { return T[(size_t)rowpos[t] * pitch + slot[i]]; };
    auto xb = [&](int t) { return T[(size_t)rowpos[t] * pitch + m]; };
    auto below = [&](int t) { return xb(t) < Lv[t] - eps; };
    auto above = [&](int t) { return Hv[t] < INFINITY && xb(t) > Hv[t] + eps; };

    const int run = d.run_status ? d.run_status[lp] : LP_OPTIMAL;
    int status = LP_OPTIMAL;   // the certificate's own
    int kind = LP_CERT_NONE, index = -1;
    const bool eligible = !d.run_status || run == LP_INFEASIBLE || run == LP_UNBOUNDED;
    if (eligible) {
        int crossed = 0, rep = 0;
        for (int j = tid; j < n; j += NT)
            if (hi[j] < lo[j]) crossed = 1;
        for (int t = tid; t < m; t += NT)
            for (int u = 0; u < t; ++u)
                if (N[u] == N[t]) rep = 1;
        if (block_any(crossed)) status = LP_INFEASIBLE;
        else if (block_any(rep)) status = LP_SINGULAR;
    }
    if (eligible && status == LP_OPTIMAL) {
        for (int j = tid; j < n; j += NT) pos[j] = up[j] ? kAtUpper : kAtLower;
        __syncthreads();
        for (int t = tid; t < m; t += NT) {
            const int k = N[t];
            if (k < n) pos[k] = t;
            Lv[t] = k < n ? lo[k] : 0.0;
            Hv[t] = k < n ? hi[k] : INFINITY;
        }
        __syncthreads();
        for (int j = tid; j < n; j += NT) vv[j] = pos[j] >= 0 ? 0.0 : pos[j] == kAtUpper ? hi[j] : lo[j];
        __syncthreads();
        // ---- b' and b0: one chain each per row, j ascending; consecutive threads, consecutive i
        for (int i = tid; i < m; i += NT) {
            double acc = b[i], b0 = b[i];
            for (int j = 0; j < n; ++j) {
                const double a = A[(size_t)j * m + i], v = vv[j], l = lo[j];
                if (v != 0.0) acc = fma(-a, v, acc);
                if (l != 0.0) b0 = fma(-a, l, b0);
            }
            bp[i] = acc;
            fv[i] = b0 < -eps ? -1.0 : 1.0;
            T[(size_t)i * pitch + m] = acc;
            used[i] = 0;
            zneg[i] = 0;
        }
        __syncthreads();
        // ---- [B | I | b'] in place: T[i][t] = column N[t] (A's, or s_i e_i for an artificial)
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m, k = N[t];
            T[(size_t)i * pitch + t] = k < n ? A[(size_t)k * m + i] : (k - n == i ? fv[i] : 0.0);
        }
        __syncthreads();
        status = ranging_crash<NT, true>(T, m, pitch, lcol, prow, used, rowpos, zneg, pub);
    }
    const bool on = eligible && status == LP_OPTIMAL;
    if (on) {
        for (int s = tid; s < m; s += NT) slot[rowpos[s]] = s;
        for (int i = tid; i < m; i += NT) used[i] = -1;   // now: the position of artificial n+i
        __syncthreads();
        int art = 0, viol = 0;
        for (int t = tid; t < m; t += NT) {
            if (N[t] >= n) {
                used[N[t] - n] = t;
                art = 1;
            } else if (below(t) || above(t)) {
                viol = 1;
            }
        }
        const bool any_art = block_any(art);
        const bool any_viol = block_any(viol);
        double* tile = U;
        if (any_art) {
            // ---- phase-I case: f, the artificials' sum, then the sign test of every f^T A_j
            for (int i = tid; i < m; i += NT) {
                double u = 0.0;
                for (int t = 0; t < m; ++t)
                    if (N[t] >= n) u = u + binv(t, i);
                fv[i] = -u;
            }
            if (tid == 0) {
                double sum = 0.0;
                for (int i = 0; i < m; ++i)
                    if (used[i] >= 0) sum = sum + xb(used[i]);
                pub[3] = sum > eps;
            }
            __syncthreads();
            bool ok = pub[3] != 0;
            const int rp[1] = {0};
            for (int j0 = 0; j0 < n && ok; j0 += kCW) {
                double g[1];
                col_chains<NT, 1>(A, m, n, j0, tile, fv, rp, nullptr, g);
                const int j = j0 + tid;
                bool fail = false;
                if (tid < kCW && j < n && pos[j] < 0) fail = pos[j] == kAtUpper ? !(g[0] <= eps) : !(g[0] >= -eps);
                ok = !block_any(fail);
            }
            if (ok) kind = LP_CERT_FARKAS;
        } else if (any_viol) {
            // ---- dual-simplex case: the violated positions in order (2t + side), kR alpha rows per pass
            if (tid == 0) {
                int q = 0;
                for (int t = 0; t < m; ++t)
                    if (below(t)) used[q++] = 2 * t;
                    else if (above(t)) used[q++] = 2 * t + 1;
                pub[3] = q;
            }
            __syncthreads();
            const int nc = pub[3];
            for (int c0 = 0; c0 < nc && kind == LP_CERT_NONE; c0 += kR) {
                int rp[kR];
                bool neg[kR];
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const int q = used[c0 + r < nc ? c0 + r : c0];
                    rp[r] = rowpos[q >> 1] * pitch;
                    neg[r] = (q & 1) != 0;
                }
                if (tid < kR) okr[tid] = 1;
                for (int j0 = 0; j0 < n; j0 += kCW) {
                    double acc[kR];
                    col_chains<NT, kR>(A, m, n, j0, tile, T, rp, slot, acc);
                    const int j = j0 + tid;
                    if (tid < kCW && j < n && pos[j] < 0) {
                        const bool flagged = pos[j] == kAtUpper;
#pragma unroll
                        for (int r = 0; r < kR; ++r) {
                            const double g = neg[r] ? -acc[r] : acc[r];
                            if (flagged ? !(g <= eps) : !(g >= -eps)) okr[r] = 0;
                        }
                    }
                }
                __syncthreads();
                for (int r = 0; r < kR && c0 + r < nc; ++r)
                    if (okr[r]) {
                        kind = LP_CERT_FARKAS;
                        index = used[c0 + r];   // 2t + side until the outputs
                        break;
                    }
                __syncthreads();   // okr: every reader is done before the next pass resets it
            }
            if (kind == LP_CERT_FARKAS) {
                const bool neg = (index & 1) != 0;
                index >>= 1;
                for (int i = tid; i < m; i += NT) fv[i] = neg ? -binv(index, i) : binv(index, i);
            }
        } else {
            // ---- ray case: per column d_j and the alpha tests over every position, kR positions per pass
            if (tid == 0) pub[3] = INT_MAX;
            double dwin = 0.0;
            for (int j0 = 0; j0 < n; j0 += kCW) {
                const int j = j0 + tid;
                const bool col = tid < kCW && j < n && pos[j] == kAtLower && hi[j] == INFINITY;
                double dj = tid < kCW && j < n ? c[j] : 0.0;
                bool ok = true;
                for (int t0 = 0; t0 < m; t0 += kR) {
                    int rp[kR];
#pragma unroll
                    for (int r = 0; r < kR; ++r) rp[r] = rowpos[t0 + r < m ? t0 + r : t0] * pitch;
                    double acc[kR];
                    col_chains<NT, kR>(A, m, n, j0, tile, T, rp, slot, acc);
#pragma unroll
                    for (int r = 0; r < kR; ++r)
                        if (t0 + r < m) {
                            dj = fma(-c[N[t0 + r]], acc[r], dj);
                            if (!(acc[r] <= eps)) ok = false;
                            if (!(acc[r] >= -eps) && Hv[t0 + r] < INFINITY) ok = false;
                        }
                }
                if (col && ok && (MX ? dj > eps : dj < -eps)) atomicMin(&pub[3], j);
                __syncthreads();
                const int w = pub[3];
                if (w != INT_MAX) {
                    if (j == w && tid < kCW) fv[0] = dj;   // (fv is free until the winner's column below)
                    __syncthreads();
                    dwin = fv[0];
                    __syncthreads();
                    kind = LP_CERT_RAY;
                    index = w;
                    break;
                }
            }
            if (kind == LP_CERT_RAY) {
                // the winner's alpha column, one chain per position, then r
                for (int t = tid; t < m; t += NT) {
                    double s = 0.0;
                    for (int i = 0; i < m; ++i) s = fma(binv(t, i), A[(size_t)index * m + i], s);
                    fv[t] = s;
                }
                __syncthreads();
                for (int k = tid; k < n; k += NT) ray[k] = k == index ? 1.0 : pos[k] >= 0 ? -fv[pos[k]] : 0.0;
                if (tid == 0) d.value[lp] = dwin;
            }
        }
    }
    // ---- outputs (f was filled by every wave: thread 0 reads all of it for b'^T f)
    __syncthreads();
    if (kind == LP_CERT_FARKAS) {
        for (int i = tid; i < m; i += NT) farkas[i] = fv[i];
        if (tid == 0) {
            double v = 0.0;
            for (int i = 0; i < m; ++i) v = fma(bp[i], fv[i], v);
            if (index >= 0) {
                if (below(index)) {
                    if (Lv[index] != 0.0) v = v - Lv[index];
                } else {
                    v = v + Hv[index];
                }
            }
            d.value[lp] = v;
        }
    } else {
        for (int i = tid; i < m; i += NT) farkas[i] = NAN;
    }
    if (kind != LP_CERT_RAY)
        for (int k = tid; k < n; k += NT) ray[k] = NAN;
    if (tid == 0) {
        if (kind == LP_CERT_NONE) d.value[lp] = NAN;
        d.kind[lp] = kind;
        d.index[lp] = index;
        d.status[lp] = !eligible ? run : status != LP_OPTIMAL ? status : run;
    }
}

template <int NT, bool MX>
int bounded_certificate_launch(lp_context* ctx, const BasisBoundedCertificateDev& d) {
    return lp_launch_per_lp(ctx, k_batched_bounded_certificate<NT, MX>, NT,
                            lp_basis_bounded_certificate_lds_bytes(d.m, d.n), d);
}

// ---- the single-LP path beyond lp_basis_bounded_certificate_fits

// Per basis position: pos (n + m, preset to -1) and, for an original column, its basic code and bounds.  The
// artificial n+i lies outside lo and hi: its L_t = 0 and H_t = +inf are never used (the dual-simplex and ray cases
// run only when no artificial is basic).
__global__ __launch_bounds__(256) void k_bcert_basic(const int* basis, int m, int n, const double* lo,
                                                     const double* hi, int* code, double* L, double* H, int* pos) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int q = basis[t];
    pos[q] = t;
    if (q < n) code[q] = kBasic;
    L[t] = q < n ? lo[q] : 0.0;
    H[t] = q < n ? hi[q] : INFINITY;
}

// T (m+1 rows, pitch ld) = [B | I | b'; 0] with artificial n+i as s_i e_i, s_i from b0; the crash bookkeeping's
// basis = 0..m-1
__global__ __launch_bounds__(256) void k_bcert_gather(SimplexDev s, const double* A, int n, const double* bp,
                                                      const double* b0, const int* basis, double eps) {
    const int i = blockIdx.x;   // tableau row, 0..m
    const int m = s.m;
    double* row = s.T + (size_t)i * s.ld;
    if (i == m) {
        for (int j = threadIdx.x; j < s.ld; j += blockDim.x) row[j] = 0.0;
        return;
    }
    const double si = b0[i] < -eps ? -1.0 : 1.0;
    for (int j = threadIdx.x; j < s.ld; j += blockDim.x) {
        double v = 0.0;
        if (j < m) v = basis[j] < n ? A[(size_t)basis[j] * m + i] : (basis[j] - n == i ? si : 0.0);
        else if (j < 2 * m) v = j - m == i ? 1.0 : 0.0;
        else if (j == 2 * m) v = bp[i];
        row[j] = v;
    }
    if (threadIdx.x == 0) s.basis[i] = i;
}

// Scratch of the single-LP reductions (device).
struct BcertScratch {
    int cas;      // 0 phase I, 1 dual simplex, 2 ray
    int ok;       // phase I: the artificials' sum > eps and no g_j has failed the sign test so far
    int best;     // ray: the first qualifying column (atomicMin), INT_MAX for none
    int pad;
};

enum { kInside = 0, kBelow = 1, kAbove = 2 };   // side[t] of an original basic column

// One block: side[t], the case, f and the sum test of phase I
__global__ __launch_bounds__(256) void k_bcert_prepare(SimplexDev s, int n, const int* basis, const double* L,
                                                       const double* H, const int* pos, double eps, int* side,
                                                       double* f, BcertScratch* cs) {
    __shared__ int flags[2];
    const int m = s.m, ld = s.ld, tid = threadIdx.x;
    if (tid == 0) flags[0] = flags[1] = 0;
    __syncthreads();
    for (int t = tid; t < m; t += 256) {
        int sd = kInside;
        if (basis[t] >= n) {
            flags[0] = 1;
        } else {
            const double xb = s.T[(size_t)t * ld + 2 * m], Lt = L[t], Ht = H[t];
            if (xb < Lt - eps) sd = kBelow;
            else if (Ht < INFINITY && xb > Ht + eps) sd = kAbove;
            if (sd != kInside) flags[1] = 1;
        }
        side[t] = sd;
    }
    __syncthreads();
    const int cas = flags[0] ? 0 : flags[1] ? 1 : 2;
    if (cas == 0)
        for (int i = tid; i < m; i += 256) {
            double u = 0.0;
            for (int t = 0; t < m; ++t)
                if (basis[t] >= n) u = u + s.T[(size_t)t * ld + m + i];
            f[i] = -u;
        }
    if (tid == 0) {
        double sum = 0.0;
        if (cas == 0)
            for (int i = 0; i < m; ++i)
                if (pos[n + i] >= 0) sum = sum + s.T[(size_t)pos[n + i] * ld + 2 * m];
        cs->cas = cas;
        cs->ok = cas == 0 && sum > eps;
        cs->best = INT_MAX;
    }
}

// the sign test of one non-basic column: g >= -eps held at lo, g <= eps held at hi (a NaN fails)
__device__ inline bool bcert_sign_ok(double g, int code, double eps) { return code == kUpper ? g <= eps : g >= -eps; }

// One thread per original column j, walking alpha down its column (coalesced across the block); what is per position
// (the violation side; c_B and whether H_t is finite) is staged through LDS 256 positions at a time.  Phase I: g_j;
// dual simplex: the sign test of every violated row (bad[t]); ray: d_j (dd[j]) and its qualification.  No thread
// leaves before the last barrier.
template <bool MX>
__global__ __launch_bounds__(256) void k_bcert_columns(SimplexDev s, const double* A, int n, const double* c,
                                                       const double* hi, const int* basis, const double* alpha,
                                                       const double* f, const int* code, const int* side,
                                                       const double* H, double eps, int* bad, double* dd,
                                                       BcertScratch* cs) {
    __shared__ double scb[256];
    __shared__ int sflag[256];
    const int m = s.m, tid = threadIdx.x;
    const int j = blockIdx.x * 256 + tid;
    const int cas = cs->cas;
    const int cj = j < n ? code[j] : kBasic;
    const bool on = cj != kBasic;   // a non-basic column inside the range
    if (cas == 0) {
        if (!on || !cs->ok) return;   // (no barrier in this case)
        double g = 0.0;
        for (int i = 0; i < m; ++i) g = fma(f[i], A[(size_t)j * m + i], g);
        if (!bcert_sign_ok(g, cj, eps)) cs->ok = 0;
        return;
    }
    if (cas == 1) {
        for (int t0 = 0; t0 < m; t0 += 256) {
            sflag[tid] = t0 + tid < m ? side[t0 + tid] : kInside;
            __syncthreads();
            const int cnt = m - t0 < 256 ? m - t0 : 256;
            if (on)
                for (int k = 0; k < cnt; ++k) {
                    const int sd = sflag[k];
                    if (sd == kInside) continue;
                    const double a = alpha[(size_t)(t0 + k) * n + j];
                    if (!bcert_sign_ok(sd == kBelow ? a : -a, cj, eps)) bad[t0 + k] = 1;
                }
            __syncthreads();
        }
        return;
    }
    double dj = j < n ? c[j] : 0.0;
    bool ok = true;
    for (int t0 = 0; t0 < m; t0 += 256) {
        const int t = t0 + tid;
        scb[tid] = t < m ? c[basis[t]] : 0.0;
        sflag[tid] = t < m ? (H[t] < INFINITY) : 0;
        __syncthreads();
        const int cnt = m - t0 < 256 ? m - t0 : 256;
        if (on)
            for (int k = 0; k < cnt; ++k) {
                const double a = alpha[(size_t)(t0 + k) * n + j];
                dj = fma(-scb[k], a, dj);
                if (!(a <= eps)) ok = false;
                if (!(a >= -eps) && sflag[k]) ok = false;
            }
        __syncthreads();
    }
    if (!on) return;
    dd[j] = dj;
    if (cj == kLower && hi[j] == INFINITY && ok && (MX ? dj > eps : dj < -eps)) atomicMin(&cs->best, j);
}

// One block: the outputs
__global__ __launch_bounds__(256) void k_bcert_finish(SimplexDev s, int n, const double* bp, const double* alpha,
                                                      const double* f, const int* pos, const int* side,
                                                      const double* L, const double* H, const int* bad,
                                                      const double* dd, const BcertScratch* cs, int* kind_out,
                                                      double* farkas, double* ray, double* value_out,
                                                      int* index_out) {
    __shared__ int pick[2];   // kind, index
    const int m = s.m, ld = s.ld, tid = threadIdx.x;
    const int cas = cs->cas;
    if (tid == 0) {
        int kind = LP_CERT_NONE, index = -1;
        if (cas == 0) {
            if (cs->ok) kind = LP_CERT_FARKAS;
        } else if (cas == 1) {
            for (int t = 0; t < m; ++t)
                if (side[t] != kInside && !bad[t]) {
                    kind = LP_CERT_FARKAS;
                    index = t;
                    break;
                }
        } else if (cs->best != INT_MAX) {
            kind = LP_CERT_RAY;
            index = cs->best;
        }
        pick[0] = kind;
        pick[1] = index;
    }
    __syncthreads();
    const int kind = pick[0], index = pick[1];
    const bool neg = kind == LP_CERT_FARKAS && cas == 1 && side[index] == kAbove;
    // f: phase I's, or row `index` of B^-1, negated above the bound
    auto fi = [&](int i) {
        if (cas == 0) return f[i];
        const double r = s.T[(size_t)index * ld + m + i];
        return neg ? -r : r;
    };
    for (int i = tid; i < m; i += 256) farkas[i] = kind == LP_CERT_FARKAS ? fi(i) : NAN;
    for (int k = tid; k < n; k += 256)
        ray[k] = kind != LP_CERT_RAY ? NAN
                 : k == index        ? 1.0
                 : pos[k] >= 0       ? -alpha[(size_t)pos[k] * n + index]
                                     : 0.0;
    if (tid == 0) {
        double v = NAN;
        if (kind == LP_CERT_FARKAS) {
            v = 0.0;
            for (int i = 0; i < m; ++i) v = fma(bp[i], fi(i), v);
            if (cas == 1) {
                if (neg) v = v + H[index];
                else if (L[index] != 0.0) v = v - L[index];
            }
        } else if (kind == LP_CERT_RAY) {
            v = dd[index];
        }
        *kind_out = kind;
        *value_out = v;
        *index_out = index;
    }
}

}  // namespace

size_t lp_basis_bounded_certificate_lds_bytes(int m, int n) {
    // pub (2 doubles), T, the scratch region, fv, b', v, L + H; rowpos + used + zneg + slot, pos, okr
    return sizeof(double) * (2 + (size_t)m * bcert_pitch(m) + bcert_scratch(m) + 4 * (size_t)m + (size_t)n) +
           sizeof(int) * (4 * (size_t)m + n + kR);
}

bool lp_basis_bounded_certificate_fits_shape(int m, int n) {
    return lp_bounded_fits_shape(m, n) && lp_basis_bounded_certificate_lds_bytes(m, n) <= 160 * 1024;
}

int lp_basis_bounded_certificate_launch(lp_context* ctx, const BasisBoundedCertificateDev& d) {
    if (!lp_basis_bounded_certificate_fits_shape(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "bounded basis certificate: the shape does not fit one CU's LDS");
    if (d.batch <= 0) return LP_OPTIMAL;
    if (bcert_threads(d.m) == 256)
        return d.maximize ? bounded_certificate_launch<256, true>(ctx, d)
                          : bounded_certificate_launch<256, false>(ctx, d);
    return d.maximize ? bounded_certificate_launch<512, true>(ctx, d)
                      : bounded_certificate_launch<512, false>(ctx, d);
}

// One LP of any shape on the device (d.batch = 1; the bounds, the flags, eps and the basis' range and repeats checked
// by the caller): every launch on the context's stream, one sync beyond the crash's own.  Returns LP_OPTIMAL (d.kind,
// d.farkas, d.ray, d.value, d.index written), LP_INFEASIBLE (crossed bounds) or LP_SINGULAR (outputs untouched);
// d.run_status is not read and d.status is not written.
int lp_basis_bounded_certificate_device(lp_context* ctx, const BasisBoundedCertificateDev& d) {
    hipStream_t s = ctx->stream;
    const int m = d.m, n = d.n;
    const int ld = (int)lp_ceil_div<size_t>(2 * (size_t)m + 1, 8) * 8;
    lp_simplex_problem q;
    q.ctx = ctx;
    q.tableau_bytes = sizeof(double) * (size_t)(m + 1) * ld;
    SimplexDev& sd = q.dev;
    sd.m = m;
    sd.n = 2 * m;   // the right-hand-side column of [B | I | b']
    sd.ld = ld;
    // one allocation: T, the pristine copy the crash permutes through, lcol, prow, state, basis, rowpos, rowused;
    // v, b', b0, L, H, the codes and the crossed-bound word; alpha, f, d, pos, side, bad and the scratch record
    double *v, *bp, *b0, *L, *H, *alpha, *f, *dd;
    int *code, *crossed, *pos, *side, *bad;
    BcertScratch* cs;
    auto pieces = [&](lp_carver& cv) {
        sd.T = cv.take<double>(q.tableau_bytes);
        q.dT0 = cv.take<double>(q.tableau_bytes);
        sd.lcol = cv.take<double>(sizeof(double) * ((size_t)m + 1));
        sd.prow = cv.take<double>(sizeof(double) * (size_t)ld);
        sd.state = cv.take<SimplexState>(sizeof(SimplexState));
        sd.basis = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowpos = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowused = cv.take<unsigned char>((size_t)m);
        v = cv.take<double>(sizeof(double) * (size_t)n);
        bp = cv.take<double>(sizeof(double) * (size_t)m);
        b0 = cv.take<double>(sizeof(double) * (size_t)m);
        L = cv.take<double>(sizeof(double) * (size_t)m);
        H = cv.take<double>(sizeof(double) * (size_t)m);
        code = cv.take<int>(sizeof(int) * (size_t)n);
        crossed = cv.take<int>(sizeof(int));
        alpha = cv.take<double>(sizeof(double) * (size_t)m * n);
        f = cv.take<double>(sizeof(double) * (size_t)m);
        dd = cv.take<double>(sizeof(double) * (size_t)n);
        pos = cv.take<int>(sizeof(int) * ((size_t)n + m));
        side = cv.take<int>(sizeof(int) * (size_t)m);
        bad = cv.take<int>(sizeof(int) * (size_t)m);
        cs = cv.take<BcertScratch>(sizeof(BcertScratch));
    };
    char* arena = nullptr;
    LP_HIP(ctx, lp_carve_malloc(&arena, pieces));
    int rc = LP_OPTIMAL, hcrossed = 0;
    hipError_t e = hipMemsetAsync(crossed, 0, sizeof(int), s);
    if (e == hipSuccess) e = hipMemsetAsync(bad, 0, sizeof(int) * (size_t)m, s);
    if (e == hipSuccess) e = hipMemsetAsync(pos, 0xff, sizeof(int) * ((size_t)n + m), s);   // -1
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bsens_codes, lp_ceil_div(n, 256), 256, 0, s, n, d.lo, d.hi, d.at_upper, code, crossed);
        hipLaunchKernelGGL(k_bcert_basic, lp_ceil_div(m, 256), 256, 0, s, d.basis, m, n, d.lo, d.hi, code, L, H, pos);
        hipLaunchKernelGGL(k_bsens_held, lp_ceil_div(n, 256), 256, 0, s, n, d.lo, d.hi, code, v);
        hipLaunchKernelGGL(k_bsens_bprime, lp_ceil_div(m, 64), 64, 0, s, d.A, m, n, d.b, v, bp);
        hipLaunchKernelGGL(k_bsens_bprime, lp_ceil_div(m, 64), 64, 0, s, d.A, m, n, d.b, d.lo, b0);   // lo held
        hipLaunchKernelGGL(k_bcert_gather, m + 1, 256, 0, s, sd, d.A, n, bp, b0, d.basis, d.eps);
        e = hipMemcpyAsync(&hcrossed, crossed, sizeof(int), hipMemcpyDeviceToHost, s);   // read after the crash's sync
    }
    if (e != hipSuccess) rc = -(int)e;
    if (rc == LP_OPTIMAL) rc = lp_simplex_crash(&q);   // m launch pairs, the verdict, rows into position order; one host sync
    if (rc >= 0 && hcrossed) rc = LP_INFEASIBLE;        // the reference checks the bounds before it pivots
    if (rc == LP_OPTIMAL) {
        lp_binv_times_a_launch(ctx, sd, d.A, n, alpha);
        hipLaunchKernelGGL(k_bcert_prepare, 1, 256, 0, s, sd, n, d.basis, L, H, pos, d.eps, side, f, cs);
        if (d.maximize)
            hipLaunchKernelGGL(k_bcert_columns<true>, lp_ceil_div(n, 256), 256, 0, s, sd, d.A, n, d.c, d.hi, d.basis,
                               alpha, f, code, side, H, d.eps, bad, dd, cs);
        else
            hipLaunchKernelGGL(k_bcert_columns<false>, lp_ceil_div(n, 256), 256, 0, s, sd, d.A, n, d.c, d.hi, d.basis,
                               alpha, f, code, side, H, d.eps, bad, dd, cs);
        hipLaunchKernelGGL(k_bcert_finish, 1, 256, 0, s, sd, n, bp, alpha, f, pos, side, L, H, bad, dd, cs, d.kind,
                           d.farkas, d.ray, d.value, d.index);
        e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->last_error = std::string("bounded basis certificate: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(arena);
    return rc;
}
