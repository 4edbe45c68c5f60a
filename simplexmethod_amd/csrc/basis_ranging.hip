// basis_ranging.hip — RHS and cost ranging at a given basis, exactly as tests/ref/ranging_ref.c states it:
//   - Binv and xB by orc_simplex_tableau's crash on [B | I | b] with the identity basis 0..m-1;
//   - d: the reduced costs of basis_duals.hip (the crash on [B^T | c_B], then one fma chain per column);
//   - alpha[t][j] = sum_i Binv[t][i] A[i][j], one fma chain per output in row order, non-basic j only;
//   - the RHS ends of row i: over t with |Binv[t][i]| > eps the ratios -xB[t] / Binv[t][i] (max for the lower
//     end, min for the upper); the cost ends of basic column basis[t]: over non-basic j with |alpha| > eps the
//     ratios d_j / alpha[t][j]; non-basic columns [-inf, c_j - d_j] (max) or [c_j - d_j, +inf] (min).
//   Every reduction keys on (value, index): the first index wins a tie, and the reported value is that index's own.
//
// k_batched_ranging: one LP per workgroup, state in LDS.  The [B^T | c_B] crash (as k_batched_duals) gives y; the
// A tiles then give d.  The [B | I | b] crash runs in place in m x (m+1): column t of B turns into a unit vector
// when it pivots and feeds nothing afterwards, so the slot takes the identity column of the pivot row.  The
// identity columns not yet pivoted are implicit: 1.0 in their own row, +0.0 in the rows not yet pivoted, and in a
// pivoted row a zero whose sign is one flag per row (zneg; tableau_pivot's fma(l, +0.0, z) keeps -0.0 only while l
// is negative).  That keeps every bit of the explicit m x (2m+1) form.  The RHS ranges are one wave per row of
// B^-1's columns; the alpha chains run kR basis positions per thread against A tiles staged through LDS.
//
// Shapes beyond lp_basis_ranging_fits: the duals path of basis_duals.hip for d; k_ranging_gather builds
// [B | I | b; 0] and the single-LP launch pair (lp_simplex_crash) pivots it; k_binv_times_a forms
// B^-1 A as tiled fp64 chains; k_rhs_ranging and k_cost_ranging reduce.
#include <cfloat>

#include "basis_crash.hpp"
#include "batched_problem.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kCW = 256;   // columns per chunk of the d and alpha passes (one per thread of a group)
constexpr int kTR = 8;     // rows of A per staged tile (64-byte segments of A's columns)
constexpr int kR = 8;      // basis positions per thread in one alpha pass

__host__ __device__ inline int ranging_threads(int m) { return m <= 64 ? 256 : 512; }
__host__ __device__ inline int ranging_pitch(int m) { return (m + 1) | 1; }
// doubles of the region that holds lcol + prow during a crash, the A tiles, then the reduction scratch
__host__ __device__ inline size_t ranging_scratch(int m) {
    const size_t tile = (size_t)kCW * (kTR + 1), eta = 2 * (size_t)m + 1;
    return tile > eta ? tile : eta;
}

template <int NT, bool MX>
__global__ __launch_bounds__(NT) void k_batched_ranging(BasisRangingDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NG = NT / kCW;   // thread groups of the alpha pass, kR basis positions each
    const int m = d.m, n = d.n, pitch = ranging_pitch(m);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    constexpr bool mx = MX;   // d.maximize, dispatched at launch
    const double eps = d.eps;
    // ---- LDS carve
    int* pub = reinterpret_cast<int*>(smem);               // [0] pivot row, [1] singular verdict, [2] block_any
    double* T = smem + 2;                                  // m x pitch
    double* U = T + (size_t)m * pitch;                     // lcol + prow | the A tiles | the reduction scratch
    double* yv = U + ranging_scratch(m);                   // m
    double* dv = yv + m;                                   // n
    int* rowpos = reinterpret_cast<int*>(dv + n);          // m
    int* used = rowpos + m;                                // m
    int* zneg = used + m;                                  // m
    int* slot = zneg + m;                                  // m: slot[i] holds identity column m+i
    int* basic = slot + m;                                 // n
    double* lcol = U;
    double* prow = U + m;

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const int* N = d.basis + (size_t)lp * m;
    double* rhs = d.rhs + (size_t)lp * 2 * m;
    int* rhs_var = d.rhs_var + (size_t)lp * 2 * m;
    double* cost = d.cost + (size_t)lp * 2 * n;
    int* cost_var = d.cost_var + (size_t)lp * 2 * n;
    constexpr int ANY_WORD = 2;   // block_any's word of pub
#include "batched_block_any.hpp"

    int status = d.run_status ? d.run_status[lp] : LP_OPTIMAL;
    if (status == LP_OPTIMAL) {
        int bad = 0;
        for (int t = tid; t < m; t += NT)
            if (N[t] < 0 || N[t] >= n) bad = 1;
        if (block_any(bad)) status = LP_BAD_ARG;
    }
    if (status == LP_OPTIMAL) {
        // ---- y: the crash on [B^T | c_B]; row t = column N[t] of A (contiguous: coalesced along i)
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m;
            T[(size_t)t * pitch + i] = A[(size_t)N[t] * m + i];
        }
        for (int t = tid; t < m; t += NT) {
            T[(size_t)t * pitch + m] = c[N[t]];
            used[t] = 0;
        }
        __syncthreads();
        status = ranging_crash<NT, false>(T, m, pitch, lcol, prow, used, rowpos, zneg, pub);
    }
    if (status == LP_OPTIMAL) {
        for (int t = tid; t < m; t += NT) yv[t] = T[(size_t)rowpos[t] * pitch + m];
        for (int j = tid; j < n; j += NT) basic[j] = 0;
        __syncthreads();
        for (int t = tid; t < m; t += NT) basic[N[t]] = 1;
        // ---- [B | I | b] in place: T[i][t] = A[i][N[t]], T[i][m] = b[i]
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m;
            T[(size_t)i * pitch + t] = A[(size_t)N[t] * m + i];
        }
        for (int i = tid; i < m; i += NT) {
            T[(size_t)i * pitch + m] = b[i];
            used[i] = 0;
            zneg[i] = 0;
        }
        __syncthreads();
        status = ranging_crash<NT, true>(T, m, pitch, lcol, prow, used, rowpos, zneg, pub);
    }
    if (status != LP_OPTIMAL) {
        for (int k = tid; k < 2 * m; k += NT) {
            rhs[k] = NAN;
            rhs_var[k] = -1;
        }
        for (int k = tid; k < 2 * n; k += NT) {
            cost[k] = NAN;
            cost_var[k] = -1;
        }
        if (tid == 0) d.status[lp] = status;
        return;
    }
    for (int s = tid; s < m; s += NT) slot[rowpos[s]] = s;
    if (tid == 0) d.status[lp] = LP_OPTIMAL;
    // ---- d = c - A^T y: tiles of kTR rows x kCW columns staged through U (column pitch kTR + 1, odd)
    double* tile = U;
    for (int j0 = 0; j0 < n; j0 += kCW) {
        const int j = j0 + tid;
        const bool on = tid < kCW && j < n;
        double s = on ? c[j] : 0.0;
        for (int i0 = 0; i0 < m; i0 += kTR) {
            const int rows = m - i0 < kTR ? m - i0 : kTR;
            for (int e = tid; e < kCW * kTR; e += NT) {
                const int cc = e / kTR, rr = e % kTR;
                if (rr < rows && j0 + cc < n) tile[cc * (kTR + 1) + rr] = A[(size_t)(j0 + cc) * m + i0 + rr];
            }
            __syncthreads();
            if (on)
                for (int rr = 0; rr < rows; ++rr) s = fma(-tile[tid * (kTR + 1) + rr], yv[i0 + rr], s);
            __syncthreads();
        }
        if (on) dv[j] = basic[j] ? 0.0 : s;
    }
    __syncthreads();
    // ---- RHS ranges: one wave per row i, over t in lanes (ascending per lane), then the (value, index) reduction
    for (int i = wave; i < m; i += NT / 64) {
        const int si = slot[i];
        double lo = 0.0, hi = 0.0;
        int klo = -1, khi = -1;
        for (int t = lane; t < m; t += 64) {
            const double* Tr = T + (size_t)rowpos[t] * pitch;
            const double beta = Tr[si];
            if (beta > eps) take<true>(-Tr[m] / beta, t, lo, klo);
            else if (beta < -eps) take<false>(-Tr[m] / beta, t, hi, khi);
        }
        wave_take<true>(lo, klo);
        wave_take<false>(hi, khi);
        if (lane == 0) {
            rhs[2 * i] = klo < 0 ? -INFINITY : b[i] + lo;
            rhs[2 * i + 1] = khi < 0 ? INFINITY : b[i] + hi;
            rhs_var[2 * i] = klo < 0 ? -1 : N[klo];
            rhs_var[2 * i + 1] = khi < 0 ? -1 : N[khi];
        }
    }
    // ---- cost ranges of the non-basic columns
    for (int j = tid; j < n; j += NT) {
        if (basic[j]) continue;
        const double e = c[j] - dv[j];
        cost[2 * j] = mx ? -INFINITY : e;
        cost[2 * j + 1] = mx ? e : INFINITY;
        cost_var[2 * j] = mx ? -1 : j;
        cost_var[2 * j + 1] = mx ? j : -1;
    }
    // ---- cost ranges of the basic columns: group g of kCW threads runs the alpha chains of kR basis positions
    // (column cj per chunk of kCW), keeping per thread the best ratio on each side across the chunks
    const int g = tid / kCW, cj = tid - g * kCW;
    double* redv = U;                                                        // [NT/64][kR][2]
    int* redk = reinterpret_cast<int*>(U + (size_t)(NT / 64) * kR * 2);   // [NT/64][kR][2]
    for (int t0 = 0; t0 < m; t0 += kR * NG) {
        int rp[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int t = t0 + g * kR + r;
            rp[r] = rowpos[t < m ? t : 0] * pitch;
        }
        double pv[kR], nv[kR];   // alpha > eps side, alpha < -eps side
        int pk[kR], nk[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            pv[r] = nv[r] = 0.0;
            pk[r] = nk[r] = -1;
        }
        for (int j0 = 0; j0 < n; j0 += kCW) {
            const int j = j0 + cj;
            double acc[kR];
#pragma unroll
            for (int r = 0; r < kR; ++r) acc[r] = 0.0;
            __syncthreads();   // U: the previous reader is done
            for (int i0 = 0; i0 < m; i0 += kTR) {
                const int rows = m - i0 < kTR ? m - i0 : kTR;
                for (int e = tid; e < kCW * kTR; e += NT) {
                    const int cc = e / kTR, rr = e % kTR;
                    if (rr < rows && j0 + cc < n) tile[cc * (kTR + 1) + rr] = A[(size_t)(j0 + cc) * m + i0 + rr];
                }
                __syncthreads();
                for (int rr = 0; rr < rows; ++rr) {
                    const double a = tile[cj * (kTR + 1) + rr];
                    const int si = slot[i0 + rr];
#pragma unroll
                    for (int r = 0; r < kR; ++r) acc[r] = fma(T[rp[r] + si], a, acc[r]);
                }
                __syncthreads();
            }
            if (j < n && !basic[j]) {
                const double dj = dv[j];
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const double s = acc[r];
                    if (s > eps) take<MX>(dj / s, j, pv[r], pk[r]);
                    else if (s < -eps) take<!MX>(dj / s, j, nv[r], nk[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            wave_take<MX>(pv[r], pk[r]);
            wave_take<!MX>(nv[r], nk[r]);
        }
        __syncthreads();   // U: the last tile's readers are done
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < kR; ++r) {
                const int q = (wave * kR + r) * 2;
                redv[q] = pv[r];
                redk[q] = pk[r];
                redv[q + 1] = nv[r];
                redk[q + 1] = nk[r];
            }
        }
        __syncthreads();
        for (int q = tid; q < NG * kR; q += NT) {
            const int gg = q / kR, r = q - gg * kR, t = t0 + q;
            if (t >= m) continue;
            double p = 0.0, v = 0.0;
            int pi = -1, vi = -1;
            for (int w = gg * (kCW / 64); w < (gg + 1) * (kCW / 64); ++w) {
                const int o = (w * kR + r) * 2;
                take<MX>(redv[o], redk[o], p, pi);
                take<!MX>(redv[o + 1], redk[o + 1], v, vi);
            }
            const double lo = mx ? p : v, hi = mx ? v : p;
            const int klo = mx ? pi : vi, khi = mx ? vi : pi;
            const int col = N[t];
            cost[2 * col] = klo < 0 ? -INFINITY : c[col] + lo;
            cost[2 * col + 1] = khi < 0 ? INFINITY : c[col] + hi;
            cost_var[2 * col] = klo;
            cost_var[2 * col + 1] = khi;
        }
    }
}

template <int NT, bool MX>
int batched_ranging_launch(lp_context* ctx, const BasisRangingDev& d) {
    return lp_launch_per_lp(ctx, k_batched_ranging<NT, MX>, NT, lp_basis_ranging_lds_bytes(d.m, d.n), d);
}

// ---- the single-LP path beyond lp_basis_ranging_fits

// T (m+1 rows, pitch ld) = [B | I | b; 0]; the crash bookkeeping's basis = 0..m-1
__global__ __launch_bounds__(256) void k_ranging_gather(SimplexDev s, const double* A, const double* b,
                                                        const int* basis) {
    const int i = blockIdx.x;   // tableau row, 0..m
    const int m = s.m;
    double* row = s.T + (size_t)i * s.ld;
    if (i == m) {
        for (int j = threadIdx.x; j < s.ld; j += blockDim.x) row[j] = 0.0;
        return;
    }
    for (int j = threadIdx.x; j < s.ld; j += blockDim.x)
        row[j] = j < m ? A[(size_t)basis[j] * m + i] : j < 2 * m ? (j - m == i ? 1.0 : 0.0) : j == 2 * m ? b[i] : 0.0;
    if (threadIdx.x == 0) s.basis[i] = i;
}

__global__ __launch_bounds__(256) void k_mark_basic(const int* basis, int m, int* basic) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) basic[basis[t]] = 1;
}

constexpr int kPT = 64;   // output tile of k_binv_times_a: kPT x kPT, 4 x 4 per thread
constexpr int kPK = 16;   // chain steps per staged tile

// alpha (m x n, row-major) = B^-1 A with B^-1 = columns m..2m-1 of the crashed tableau (rows in position order):
// alpha[t][j] is the chain fma(Binv[t][i], A[i][j], s) over i ascending from 0.
__global__ __launch_bounds__(256) void k_binv_times_a(SimplexDev s, const double* A, int n, double* alpha) {
    __shared__ double Bs[kPK][kPT + 1];
    __shared__ double As[kPK][kPT + 1];
    const int m = s.m, ld = s.ld;
    const int t0 = blockIdx.y * kPT, j0 = blockIdx.x * kPT;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[a][q] = 0.0;
    for (int i0 = 0; i0 < m; i0 += kPK) {
        const int ks = m - i0 < kPK ? m - i0 : kPK;
        for (int e = tid; e < kPT * kPK; e += 256) {
            const int r = e / kPK, k = e % kPK;   // consecutive threads: consecutive i
            const int t = t0 + r, j = j0 + r;
            Bs[k][r] = (k < ks && t < m) ? s.T[(size_t)t * ld + m + i0 + k] : 0.0;
            As[k][r] = (k < ks && j < n) ? A[(size_t)j * m + i0 + k] : 0.0;
        }
        __syncthreads();
        for (int k = 0; k < ks; ++k) {
            double bv[4], av[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) bv[a] = Bs[k][ty + 16 * a];
#pragma unroll
            for (int q = 0; q < 4; ++q) av[q] = As[k][tx + 16 * q];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[a][q] = fma(bv[a], av[q], acc[a][q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int t = t0 + ty + 16 * a;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + tx + 16 * q;
            if (t < m && j < n) alpha[(size_t)t * n + j] = acc[a][q];
        }
    }
}

// RHS ranges: 64 rows i per block (lanes), four interleaved subsets of t (threadIdx.y), ascending in each
__global__ __launch_bounds__(256) void k_rhs_ranging(SimplexDev s, const double* b, const int* basis, double eps,
                                                     double* rhs, int* rhs_var) {
    __shared__ double sv[2][4][64];
    __shared__ int sk[2][4][64];
    const int m = s.m, ld = s.ld;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i = blockIdx.x * 64 + tx;
    double lo = 0.0, hi = 0.0;
    int klo = -1, khi = -1;
    if (i < m)
        for (int t = ty; t < m; t += 4) {
            const double* Tr = s.T + (size_t)t * ld;
            const double beta = Tr[m + i];
            if (beta > eps) take<true>(-Tr[2 * m] / beta, t, lo, klo);
            else if (beta < -eps) take<false>(-Tr[2 * m] / beta, t, hi, khi);
        }
    sv[0][ty][tx] = lo;
    sk[0][ty][tx] = klo;
    sv[1][ty][tx] = hi;
    sk[1][ty][tx] = khi;
    __syncthreads();
    if (ty != 0 || i >= m) return;
    for (int y = 1; y < 4; ++y) {
        take<true>(sv[0][y][tx], sk[0][y][tx], lo, klo);
        take<false>(sv[1][y][tx], sk[1][y][tx], hi, khi);
    }
    rhs[2 * i] = klo < 0 ? -INFINITY : b[i] + lo;
    rhs[2 * i + 1] = khi < 0 ? INFINITY : b[i] + hi;
    rhs_var[2 * i] = klo < 0 ? -1 : basis[klo];
    rhs_var[2 * i + 1] = khi < 0 ? -1 : basis[khi];
}

// cost ranges: blocks 0..m-1 reduce row t of alpha over the non-basic columns; the blocks after them write the
// non-basic columns' ends
template <bool MX>
__global__ __launch_bounds__(256) void k_cost_ranging(const double* alpha, int m, int n, const double* c,
                                                      const double* dd, const int* basis, const int* basic,
                                                      double eps, double* cost, int* cost_var) {
    __shared__ double sv[2][4];
    __shared__ int sk[2][4];
    constexpr bool mx = MX;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= m) {
        const int j = (blockIdx.x - m) * 256 + tid;
        if (j >= n || basic[j]) return;
        const double e = c[j] - dd[j];
        cost[2 * j] = mx ? -INFINITY : e;
        cost[2 * j + 1] = mx ? e : INFINITY;
        cost_var[2 * j] = mx ? -1 : j;
        cost_var[2 * j + 1] = mx ? j : -1;
        return;
    }
    const int t = blockIdx.x;
    const double* ar = alpha + (size_t)t * n;
    double p = 0.0, v = 0.0;
    int pi = -1, vi = -1;
    for (int j = tid; j < n; j += 256) {
        if (basic[j]) continue;
        const double s = ar[j];
        if (s > eps) take<MX>(dd[j] / s, j, p, pi);
        else if (s < -eps) take<!MX>(dd[j] / s, j, v, vi);
    }
    wave_take<MX>(p, pi);
    wave_take<!MX>(v, vi);
    if (lane == 0) {
        sv[0][wave] = p;
        sk[0][wave] = pi;
        sv[1][wave] = v;
        sk[1][wave] = vi;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < 4; ++w) {
        take<MX>(sv[0][w], sk[0][w], p, pi);
        take<!MX>(sv[1][w], sk[1][w], v, vi);
    }
    const double lo = mx ? p : v, hi = mx ? v : p;
    const int klo = mx ? pi : vi, khi = mx ? vi : pi;
    const int col = basis[t];
    cost[2 * col] = klo < 0 ? -INFINITY : c[col] + lo;
    cost[2 * col + 1] = khi < 0 ? INFINITY : c[col] + hi;
    cost_var[2 * col] = klo;
    cost_var[2 * col + 1] = khi;
}

}  // namespace

size_t lp_basis_ranging_lds_bytes(int m, int n) {
    // pub (2 doubles), T, the scratch region, yv, dv; rowpos + used + zneg + slot, basic
    return sizeof(double) * (2 + (size_t)m * ranging_pitch(m) + ranging_scratch(m) + (size_t)m + n) +
           sizeof(int) * (4 * (size_t)m + n);
}

int lp_basis_ranging_launch(lp_context* ctx, const BasisRangingDev& d) {
    if (!lp_basis_ranging_fits(d.m, d.n)) LP_FAIL(ctx, LP_BAD_ARG, "basis ranging: the shape does not fit one CU's LDS");
    if (d.batch <= 0) return LP_OPTIMAL;
    if (ranging_threads(d.m) == 256)
        return d.maximize ? batched_ranging_launch<256, true>(ctx, d) : batched_ranging_launch<256, false>(ctx, d);
    return d.maximize ? batched_ranging_launch<512, true>(ctx, d) : batched_ranging_launch<512, false>(ctx, d);
}

// One LP of any size on the device: A, b, c, basis already there (basis range checked by the caller).
int lp_basis_ranging_device(lp_context* ctx, const double* dA, int m, int n, const double* db, const double* dc,
                            const int* dbasis, int maximize, double eps, double* drhs, int* drhs_var, double* dcost,
                            int* dcost_var) {
    hipStream_t s = ctx->stream;
    const int ld = (int)lp_ceil_div<size_t>(2 * (size_t)m + 1, 8) * 8;
    lp_simplex_problem q;
    q.ctx = ctx;
    q.tableau_bytes = sizeof(double) * (size_t)(m + 1) * ld;
    SimplexDev& sd = q.dev;
    sd.m = m;
    sd.n = 2 * m;   // the right-hand-side column of [B | I | b]
    sd.ld = ld;
    // one allocation: T, the pristine copy the crash permutes through, lcol, prow, state, basis, rowpos, rowused;
    // alpha, y, d, w and the basic flags
    double *alpha, *dy, *dd, *dw;
    int* basic;
    auto pieces = [&](lp_carver& cv) {
        sd.T = cv.take<double>(q.tableau_bytes);
        q.dT0 = cv.take<double>(q.tableau_bytes);
        sd.lcol = cv.take<double>(sizeof(double) * ((size_t)m + 1));
        sd.prow = cv.take<double>(sizeof(double) * (size_t)ld);
        sd.state = cv.take<SimplexState>(sizeof(SimplexState));
        sd.basis = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowpos = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowused = cv.take<unsigned char>((size_t)m);
        alpha = cv.take<double>(sizeof(double) * (size_t)m * n);
        dy = cv.take<double>(sizeof(double) * (size_t)m);
        dd = cv.take<double>(sizeof(double) * (size_t)n);
        dw = cv.take<double>(sizeof(double));
        basic = cv.take<int>(sizeof(int) * (size_t)n);
    };
    char* arena = nullptr;
    LP_HIP(ctx, lp_carve_malloc(&arena, pieces));
    int rc = LP_OPTIMAL;
    hipError_t e = hipMemsetAsync(basic, 0, sizeof(int) * (size_t)n, s);
    if (e != hipSuccess) rc = -(int)e;
    if (rc == LP_OPTIMAL) {
        hipLaunchKernelGGL(k_ranging_gather, m + 1, 256, 0, s, sd, dA, db, dbasis);
        rc = lp_simplex_crash(&q);   // m launch pairs, the verdict, rows into position order; one host sync
    }
    if (rc == LP_OPTIMAL) rc = lp_basis_duals_device(ctx, dA, m, n, db, dc, dbasis, dy, dd, dw);
    if (rc == LP_OPTIMAL) {
        hipLaunchKernelGGL(k_mark_basic, lp_ceil_div(m, 256), 256, 0, s, dbasis, m, basic);
        hipLaunchKernelGGL(k_binv_times_a, dim3(lp_ceil_div(n, kPT), lp_ceil_div(m, kPT)), 256, 0, s, sd, dA, n,
                           alpha);
        hipLaunchKernelGGL(k_rhs_ranging, lp_ceil_div(m, 64), dim3(64, 4), 0, s, sd, db, dbasis, eps, drhs, drhs_var);
        if (maximize)
            hipLaunchKernelGGL(k_cost_ranging<true>, m + lp_ceil_div(n, 256), 256, 0, s, alpha, m, n, dc, dd, dbasis,
                               basic, eps, dcost, dcost_var);
        else
            hipLaunchKernelGGL(k_cost_ranging<false>, m + lp_ceil_div(n, 256), 256, 0, s, alpha, m, n, dc, dd, dbasis,
                               basic, eps, dcost, dcost_var);
        e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->last_error = std::string("basis ranging: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(arena);
    return rc;
}

// B^-1 A (m x n, row-major) from a tableau lp_simplex_crash left in position order (basis_certificate.hip's
// single-LP path); queued on the context's stream, no sync.
void lp_binv_times_a_launch(lp_context* ctx, const SimplexDev& s, const double* dA, int n, double* alpha) {
    hipLaunchKernelGGL(k_binv_times_a, dim3(lp_ceil_div(n, kPT), lp_ceil_div(s.m, kPT)), 256, 0, ctx->stream, s, dA,
                       n, alpha);
}
