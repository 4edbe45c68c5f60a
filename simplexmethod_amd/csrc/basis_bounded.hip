// basis_bounded.hip — the dual solution and RHS / cost ranging of a bounded-variable LP (A x = b, lo <= x <= hi) at a
// given basis and given at-upper flags, exactly as tests/ref/bounded_sens_ref.c states them, in the caller's original
// variables:
//   - a non-basic column is held at v_j = hi_j (flagged) or lo_j; the flags of basic columns are not read;
//   - b' = b - sum_j A_j v_j: one fma chain per row over the non-basic j ascending with v_j != 0.0;
//   - y and d as basis_duals.hip (the crash on [B^T | c_B], then one fma chain per column);
//   - xB and Binv by the crash on [B | I | b'] (basis_crash.hpp, in place); x = xB on the basis, v elsewhere;
//   - w = b^T y continued over the non-basic j with v_j != 0.0 as fma(d_j, v_j, s);
//   - the RHS ends of row i: over t with |Binv[t][i]| > eps the ratios (L_t - xB[t]) / beta and, H_t finite,
//     (H_t - xB[t]) / beta, each to the end its sign moves (max for the lower end, min for the upper); reported with
//     the leaving variable and the bound it leaves at;
//   - the cost ends: the sense of a non-basic j is maximize XOR at_upper[j]; non-basic columns one finite end
//     c_j - d_j, basic columns the ratios d_j / alpha[t][j] over the non-basic j with |alpha| > eps.
//   Every reduction keys on (value, index) with its direction fixed at compile time: the lower end is always a max,
//   the upper end always a min; which of the two a candidate goes to is the only run-time choice.
//
// k_batched_bounded_sens<NT, RANGING>: one LP per workgroup, state in LDS, the structure of k_batched_ranging plus v
// (n) and the basic columns' L, H (2m).  RANGING = false is the duals entry: its second crash is [B | b'] without the
// identity block (tableau_pivot treats every column on its own, so xB has the same bits).
//
// Shapes beyond lp_basis_bounded_fits (lp_basis_bounded_device, one LP): the column codes, the held values and b' by
// small kernels; k_bsens_gather builds [B | I | b'; 0] ([B | b'; 0] for the duals) and the single-LP launch pair
// (lp_simplex_crash) pivots it; y, d and b.y by lp_basis_duals_device; then x and w, or k_binv_times_a
// (basis_ranging.hip) and the two reduction kernels.
#include <cfloat>

#include "basis_bounded_kernels.hpp"
#include "basis_crash.hpp"
#include "batched_problem.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kCW = 256;   // columns per chunk of the d and alpha passes (one per thread of a group)
constexpr int kTR = 8;     // rows of A per staged tile (64-byte segments of A's columns)
constexpr int kR = 8;      // basis positions per thread in one alpha pass

__host__ __device__ inline int bsens_threads(int m) { return m <= 64 ? 256 : 512; }
__host__ __device__ inline int bsens_pitch(int m) { return (m + 1) | 1; }
// doubles of the region that holds lcol + prow during a crash, the A tiles, then the reduction scratch
__host__ __device__ inline size_t bsens_scratch(int m) {
    const size_t tile = (size_t)kCW * (kTR + 1), eta = 2 * (size_t)m + 1;
    return tile > eta ? tile : eta;
}

template <int NT, bool RANGING>
__global__ __launch_bounds__(NT) void k_batched_bounded_sens(BasisBoundedDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NG = NT / kCW;   // thread groups of the alpha pass, kR basis positions each
    const int m = d.m, n = d.n, pitch = bsens_pitch(m);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    const bool mx = d.maximize != 0;
    const double eps = d.eps;
    // ---- LDS carve
    int* pub = reinterpret_cast<int*>(smem);               // [0] pivot row, [1] singular verdict, [2] block_any
    double* T = smem + 2;                                  // m x pitch
    double* U = T + (size_t)m * pitch;                     // lcol + prow | the A tiles | the reduction scratch
    double* yv = U + bsens_scratch(m);                     // m
    double* dv = yv + m;                                   // n
    double* vv = dv + n;                                   // n: the held values (0.0 for basic columns)
    double* Lv = vv + n;                                   // m: lo of the basic columns by position
    double* Hv = Lv + m;                                   // m: hi of the basic columns by position
    int* rowpos = reinterpret_cast<int*>(Hv + m);          // m
    int* used = rowpos + m;                                // m
    int* zneg = used + m;                                  // m
    int* slot = zneg + m;                                  // m: slot[i] holds identity column m+i
    int* code = slot + m;                                  // n: kLower / kBasic / kUpper
    double* lcol = U;
    double* prow = U + m;

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* lo = d.lo + (size_t)lp * n;
    const double* hi = d.hi + (size_t)lp * n;
    const int* N = d.basis + (size_t)lp * m;
    const int* up = d.at_upper + (size_t)lp * n;
    constexpr int ANY_WORD = 2;   // block_any's word of pub
#include "batched_block_any.hpp"

    int status = LP_OPTIMAL;
    {
        int crossed = 0;
        for (int j = tid; j < n; j += NT)
            if (hi[j] < lo[j]) crossed = 1;
        if (block_any(crossed)) status = LP_INFEASIBLE;
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
        for (int j = tid; j < n; j += NT) code[j] = up[j] ? kUpper : kLower;
        __syncthreads();
        for (int t = tid; t < m; t += NT) {
            code[N[t]] = kBasic;
            Lv[t] = lo[N[t]];
            Hv[t] = hi[N[t]];
        }
        __syncthreads();
        for (int j = tid; j < n; j += NT) vv[j] = code[j] == kBasic ? 0.0 : code[j] == kUpper ? hi[j] : lo[j];
        // ---- [B | b'] (RANGING: standing for [B | I | b'], in place): T[i][t] = A[i][N[t]], T[i][m] = b'[i]
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m;
            T[(size_t)i * pitch + t] = A[(size_t)N[t] * m + i];
        }
        __syncthreads();
        for (int i = tid; i < m; i += NT) {   // one chain per row, j ascending; consecutive threads, consecutive i
            double acc = b[i];
            for (int j = 0; j < n; ++j) {
                const double v = vv[j];
                if (v != 0.0) acc = fma(-A[(size_t)j * m + i], v, acc);
            }
            T[(size_t)i * pitch + m] = acc;
            used[i] = 0;
            zneg[i] = 0;
        }
        __syncthreads();
        status = ranging_crash<NT, RANGING>(T, m, pitch, lcol, prow, used, rowpos, zneg, pub);
    }
    if (status != LP_OPTIMAL) {
        if (RANGING) {
            double* rhs = d.rhs + (size_t)lp * 2 * m;
            double* cost = d.cost + (size_t)lp * 2 * n;
            int* rhs_var = d.rhs_var + (size_t)lp * 2 * m;
            int* rhs_side = d.rhs_side + (size_t)lp * 2 * m;
            int* cost_var = d.cost_var + (size_t)lp * 2 * n;
            for (int k = tid; k < 2 * m; k += NT) {
                rhs[k] = NAN;
                rhs_var[k] = -1;
                rhs_side[k] = -1;
            }
            for (int k = tid; k < 2 * n; k += NT) {
                cost[k] = NAN;
                cost_var[k] = -1;
            }
        } else {
            for (int j = tid; j < n; j += NT) d.x[(size_t)lp * n + j] = d.d[(size_t)lp * n + j] = NAN;
            for (int t = tid; t < m; t += NT) d.y[(size_t)lp * m + t] = NAN;
            if (tid == 0) d.w[lp] = NAN;
        }
        if (tid == 0) d.status[lp] = status;
        return;
    }
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
        if (on) dv[j] = code[j] == kBasic ? 0.0 : s;
    }
    __syncthreads();
    if (!RANGING) {
        double* x = d.x + (size_t)lp * n;
        double* dd = d.d + (size_t)lp * n;
        double* y = d.y + (size_t)lp * m;
        for (int j = tid; j < n; j += NT) {
            if (code[j] != kBasic) x[j] = vv[j];
            dd[j] = dv[j];
        }
        for (int t = tid; t < m; t += NT) {
            x[N[t]] = T[(size_t)rowpos[t] * pitch + m];
            y[t] = yv[t];
            U[t] = b[t];   // the tiles are done
        }
        __syncthreads();
        if (tid == 0) {   // w: one chain, the rows then the held non-basic columns
            double s = 0.0;
            for (int i = 0; i < m; ++i) s = fma(U[i], yv[i], s);
            for (int j = 0; j < n; ++j) {
                const double v = vv[j];
                if (v != 0.0) s = fma(dv[j], v, s);
            }
            d.w[lp] = s;
        }
        return;
    }
    double* rhs = d.rhs + (size_t)lp * 2 * m;
    double* cost = d.cost + (size_t)lp * 2 * n;
    int* rhs_var = d.rhs_var + (size_t)lp * 2 * m;
    int* rhs_side = d.rhs_side + (size_t)lp * 2 * m;
    int* cost_var = d.cost_var + (size_t)lp * 2 * n;
    for (int s = tid; s < m; s += NT) slot[rowpos[s]] = s;
    __syncthreads();
    // ---- RHS ranges: one wave per row i, over t in lanes (ascending per lane), then the (value, key) reduction.
    // The key of position t's candidate is 2t + side: a position has at most one candidate per end, so the key orders
    // as t does and carries the bound the variable leaves at.
    for (int i = wave; i < m; i += NT / 64) {
        const int si = slot[i];
        double dl = 0.0, dh = 0.0;
        int kl = -1, kh = -1;
        for (int t = lane; t < m; t += 64) {
            const double* Tr = T + (size_t)rowpos[t] * pitch;
            const double beta = Tr[si], xb = Tr[m], L = Lv[t], H = Hv[t];
            const double nL = (L == 0.0) ? -xb : L - xb, nH = H - xb;
            if (beta > eps) {
                take<true>(nL / beta, 2 * t, dl, kl);
                if (H < INFINITY) take<false>(nH / beta, 2 * t + 1, dh, kh);
            } else if (beta < -eps) {
                take<false>(nL / beta, 2 * t, dh, kh);
                if (H < INFINITY) take<true>(nH / beta, 2 * t + 1, dl, kl);
            }
        }
        wave_take<true>(dl, kl);
        wave_take<false>(dh, kh);
        if (lane == 0) {
            rhs[2 * i] = kl < 0 ? -INFINITY : b[i] + dl;
            rhs[2 * i + 1] = kh < 0 ? INFINITY : b[i] + dh;
            rhs_var[2 * i] = kl < 0 ? -1 : N[kl >> 1];
            rhs_var[2 * i + 1] = kh < 0 ? -1 : N[kh >> 1];
            rhs_side[2 * i] = kl < 0 ? -1 : (kl & 1);
            rhs_side[2 * i + 1] = kh < 0 ? -1 : (kh & 1);
        }
    }
    // ---- cost ranges of the non-basic columns
    for (int j = tid; j < n; j += NT) {
        if (code[j] == kBasic) continue;
        const bool mxj = mx != (code[j] == kUpper);
        const double e = c[j] - dv[j];
        cost[2 * j] = mxj ? -INFINITY : e;
        cost[2 * j + 1] = mxj ? e : INFINITY;
        cost_var[2 * j] = mxj ? -1 : j;
        cost_var[2 * j + 1] = mxj ? j : -1;
    }
    // ---- cost ranges of the basic columns: group g of kCW threads runs the alpha chains of kR basis positions
    // (column cj per chunk of kCW), keeping per thread the best ratio of each end across the chunks
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
        double lv[kR], hv[kR];   // lower end (max), upper end (min)
        int lk[kR], hk[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            lv[r] = hv[r] = 0.0;
            lk[r] = hk[r] = -1;
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
            if (j < n && code[j] != kBasic) {
                const double dj = dv[j];
                const bool mxj = mx != (code[j] == kUpper);
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const double s = acc[r];
                    if (!(s > eps) && !(s < -eps)) continue;
                    if ((s > eps) == mxj) take<true>(dj / s, j, lv[r], lk[r]);
                    else take<false>(dj / s, j, hv[r], hk[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            wave_take<true>(lv[r], lk[r]);
            wave_take<false>(hv[r], hk[r]);
        }
        __syncthreads();   // U: the last tile's readers are done
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < kR; ++r) {
                const int q = (wave * kR + r) * 2;
                redv[q] = lv[r];
                redk[q] = lk[r];
                redv[q + 1] = hv[r];
                redk[q + 1] = hk[r];
            }
        }
        __syncthreads();
        for (int q = tid; q < NG * kR; q += NT) {
            const int gg = q / kR, r = q - gg * kR, t = t0 + q;
            if (t >= m) continue;
            double dl = 0.0, dh = 0.0;
            int kl = -1, kh = -1;
            for (int w = gg * (kCW / 64); w < (gg + 1) * (kCW / 64); ++w) {
                const int o = (w * kR + r) * 2;
                take<true>(redv[o], redk[o], dl, kl);
                take<false>(redv[o + 1], redk[o + 1], dh, kh);
            }
            const int col = N[t];
            cost[2 * col] = kl < 0 ? -INFINITY : c[col] + dl;
            cost[2 * col + 1] = kh < 0 ? INFINITY : c[col] + dh;
            cost_var[2 * col] = kl;
            cost_var[2 * col + 1] = kh;
        }
    }
}

template <int NT, bool RANGING>
int bounded_sens_launch(lp_context* ctx, const BasisBoundedDev& d) {
    return lp_launch_per_lp(ctx, k_batched_bounded_sens<NT, RANGING>, NT, lp_basis_bounded_lds_bytes(d.m, d.n), d);
}

// ---- the single-LP path beyond lp_basis_bounded_fits

// (k_bsens_codes, k_bsens_held and k_bsens_bprime: basis_bounded_kernels.hpp)

__global__ __launch_bounds__(256) void k_bsens_basic(const int* basis, int m, const double* lo, const double* hi,
                                                     int* code, double* L, double* H) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int q = basis[t];
    code[q] = kBasic;
    L[t] = lo[q];
    H[t] = hi[q];
}

// T (m+1 rows, pitch ld) = [B | I | b'; 0] when s.n = 2m, [B | b'; 0] when s.n = m; the crash bookkeeping's
// basis = 0..m-1
__global__ __launch_bounds__(256) void k_bsens_gather(SimplexDev s, const double* A, const double* bp,
                                                      const int* basis) {
    const int i = blockIdx.x;   // tableau row, 0..m
    const int m = s.m;
    double* row = s.T + (size_t)i * s.ld;
    if (i == m) {
        for (int j = threadIdx.x; j < s.ld; j += blockDim.x) row[j] = 0.0;
        return;
    }
    for (int j = threadIdx.x; j < s.ld; j += blockDim.x)
        row[j] = j < m ? A[(size_t)basis[j] * m + i] : j == s.n ? bp[i] : j < s.n ? (j - m == i ? 1.0 : 0.0) : 0.0;
    if (threadIdx.x == 0) s.basis[i] = i;
}

// x = v on the non-basic columns, xB (the crashed tableau's right-hand column, rows in position order) on the basis
__global__ __launch_bounds__(256) void k_bsens_x(SimplexDev s, int n, const int* basis, const int* code,
                                                 const double* v, double* x) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n && code[j] != kBasic) x[j] = v[j];
    if (j < s.m) x[basis[j]] = s.T[(size_t)j * s.ld + s.n];
}

// w: b.y (already in *w) continued over j ascending with v_j != 0.0 as fma(d_j, v_j, s).  One block: the chunks of d
// and v are staged by all threads, thread 0 runs the chain.
__global__ __launch_bounds__(256) void k_bsens_w(int n, const double* dd, const double* v, double* w) {
    __shared__ double sd[256];
    __shared__ double sv[256];
    const int tid = threadIdx.x;
    double s = tid == 0 ? *w : 0.0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + tid;
        sd[tid] = j < n ? dd[j] : 0.0;
        sv[tid] = j < n ? v[j] : 0.0;
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < 256; ++k)
                if (sv[k] != 0.0) s = fma(sd[k], sv[k], s);
        __syncthreads();
    }
    if (tid == 0) *w = s;
}

// RHS ranges: 64 rows i per block (lanes), four interleaved subsets of t (threadIdx.y), ascending in each.  The key
// of position t's candidate is 2t + side, as in k_batched_bounded_sens: within a subset and across the subsets the
// smallest key of a tie is the first position.
__global__ __launch_bounds__(256) void k_bsens_rhs_ranging(SimplexDev s, const double* b, const int* basis,
                                                           const double* Lv, const double* Hv, double eps,
                                                           double* rhs, int* rhs_var, int* rhs_side) {
    __shared__ double sv[2][4][64];
    __shared__ int sk[2][4][64];
    const int m = s.m, ld = s.ld;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i = blockIdx.x * 64 + tx;
    double dl = 0.0, dh = 0.0;
    int kl = -1, kh = -1;
    if (i < m)
        for (int t = ty; t < m; t += 4) {
            const double* Tr = s.T + (size_t)t * ld;
            const double beta = Tr[m + i], xb = Tr[2 * m], L = Lv[t], H = Hv[t];
            const double nL = (L == 0.0) ? -xb : L - xb, nH = H - xb;
            if (beta > eps) {
                take<true>(nL / beta, 2 * t, dl, kl);
                if (H < INFINITY) take<false>(nH / beta, 2 * t + 1, dh, kh);
            } else if (beta < -eps) {
                take<false>(nL / beta, 2 * t, dh, kh);
                if (H < INFINITY) take<true>(nH / beta, 2 * t + 1, dl, kl);
            }
        }
    sv[0][ty][tx] = dl;
    sk[0][ty][tx] = kl;
    sv[1][ty][tx] = dh;
    sk[1][ty][tx] = kh;
    __syncthreads();
    if (ty != 0 || i >= m) return;
    for (int y = 1; y < 4; ++y) {
        take<true>(sv[0][y][tx], sk[0][y][tx], dl, kl);
        take<false>(sv[1][y][tx], sk[1][y][tx], dh, kh);
    }
    rhs[2 * i] = kl < 0 ? -INFINITY : b[i] + dl;
    rhs[2 * i + 1] = kh < 0 ? INFINITY : b[i] + dh;
    rhs_var[2 * i] = kl < 0 ? -1 : basis[kl >> 1];
    rhs_var[2 * i + 1] = kh < 0 ? -1 : basis[kh >> 1];
    rhs_side[2 * i] = kl < 0 ? -1 : (kl & 1);
    rhs_side[2 * i + 1] = kh < 0 ? -1 : (kh & 1);
}

// cost ranges: blocks 0..m-1 reduce row t of alpha over the non-basic columns (the lower end a max, the upper end a
// min; the column's sense picks the end); the blocks after them write the non-basic columns' ends
__global__ __launch_bounds__(256) void k_bsens_cost_ranging(const double* alpha, int m, int n, const double* c,
                                                            const double* dd, const int* basis, const int* code,
                                                            int maximize, double eps, double* cost, int* cost_var) {
    __shared__ double sv[2][4];
    __shared__ int sk[2][4];
    const bool mx = maximize != 0;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if ((int)blockIdx.x >= m) {
        const int j = (blockIdx.x - m) * 256 + tid;
        if (j >= n || code[j] == kBasic) return;
        const bool mxj = mx != (code[j] == kUpper);
        const double e = c[j] - dd[j];
        cost[2 * j] = mxj ? -INFINITY : e;
        cost[2 * j + 1] = mxj ? e : INFINITY;
        cost_var[2 * j] = mxj ? -1 : j;
        cost_var[2 * j + 1] = mxj ? j : -1;
        return;
    }
    const int t = blockIdx.x;
    const double* ar = alpha + (size_t)t * n;
    double dl = 0.0, dh = 0.0;
    int kl = -1, kh = -1;
    for (int j = tid; j < n; j += 256) {
        if (code[j] == kBasic) continue;
        const double s = ar[j];
        if (!(s > eps) && !(s < -eps)) continue;
        const bool mxj = mx != (code[j] == kUpper);
        if ((s > eps) == mxj) take<true>(dd[j] / s, j, dl, kl);
        else take<false>(dd[j] / s, j, dh, kh);
    }
    wave_take<true>(dl, kl);
    wave_take<false>(dh, kh);
    if (lane == 0) {
        sv[0][wave] = dl;
        sk[0][wave] = kl;
        sv[1][wave] = dh;
        sk[1][wave] = kh;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < 4; ++w) {
        take<true>(sv[0][w], sk[0][w], dl, kl);
        take<false>(sv[1][w], sk[1][w], dh, kh);
    }
    const int col = basis[t];
    cost[2 * col] = kl < 0 ? -INFINITY : c[col] + dl;
    cost[2 * col + 1] = kh < 0 ? INFINITY : c[col] + dh;
    cost_var[2 * col] = kl;
    cost_var[2 * col + 1] = kh;
}

}  // namespace

size_t lp_basis_bounded_lds_bytes(int m, int n) {
    // pub (2 doubles), T, the scratch region, yv, dv, v, L + H; rowpos + used + zneg + slot, code
    return sizeof(double) * (2 + (size_t)m * bsens_pitch(m) + bsens_scratch(m) + 3 * (size_t)m + 2 * (size_t)n) +
           sizeof(int) * (4 * (size_t)m + n);
}

bool lp_basis_bounded_fits_shape(int m, int n) {
    return lp_bounded_fits_shape(m, n) && lp_basis_bounded_lds_bytes(m, n) <= 160 * 1024;
}

int lp_basis_bounded_launch(lp_context* ctx, const BasisBoundedDev& d, bool ranging) {
    if (!lp_basis_bounded_fits_shape(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "bounded basis analysis: the shape does not fit one CU's LDS");
    if (d.batch <= 0) return LP_OPTIMAL;
    if (bsens_threads(d.m) == 256)
        return ranging ? bounded_sens_launch<256, true>(ctx, d) : bounded_sens_launch<256, false>(ctx, d);
    return ranging ? bounded_sens_launch<512, true>(ctx, d) : bounded_sens_launch<512, false>(ctx, d);
}

// One LP of any shape on the device (d.batch = 1; the bounds, basis and flags checked by the caller, eps >= 0): every
// launch on the context's stream, one sync beyond the two crashes' own.  Returns LP_OPTIMAL (the duals outputs, or
// with `ranging` the ranging outputs, written), LP_INFEASIBLE or LP_SINGULAR (outputs untouched); d.status is not
// written.
int lp_basis_bounded_device(lp_context* ctx, const BasisBoundedDev& d, bool ranging) {
    hipStream_t s = ctx->stream;
    const int m = d.m, n = d.n;
    const int cols = ranging ? 2 * m : m;   // the right-hand-side column of [B | I | b'] or [B | b']
    const int ld = (int)lp_ceil_div<size_t>((size_t)cols + 1, 8) * 8;
    lp_simplex_problem q;
    q.ctx = ctx;
    q.tableau_bytes = sizeof(double) * (size_t)(m + 1) * ld;
    SimplexDev& sd = q.dev;
    sd.m = m;
    sd.n = cols;
    sd.ld = ld;
    // one allocation: T, the pristine copy the crash permutes through, lcol, prow, state, basis, rowpos, rowused;
    // v, b', L, H, the codes and the crossed-bound word; for ranging alpha, y, d and b.y as well
    double *v, *bp, *L, *H, *alpha = nullptr, *dy = d.y, *dd = d.d, *dw = d.w;
    int *code, *crossed;
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
        L = cv.take<double>(sizeof(double) * (size_t)m);
        H = cv.take<double>(sizeof(double) * (size_t)m);
        code = cv.take<int>(sizeof(int) * (size_t)n);
        crossed = cv.take<int>(sizeof(int));
        if (!ranging) return;
        alpha = cv.take<double>(sizeof(double) * (size_t)m * n);
        dy = cv.take<double>(sizeof(double) * (size_t)m);
        dd = cv.take<double>(sizeof(double) * (size_t)n);
        dw = cv.take<double>(sizeof(double));
    };
    char* arena = nullptr;
    LP_HIP(ctx, lp_carve_malloc(&arena, pieces));
    int rc = LP_OPTIMAL, hcrossed = 0;
    hipError_t e = hipMemsetAsync(crossed, 0, sizeof(int), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bsens_codes, lp_ceil_div(n, 256), 256, 0, s, n, d.lo, d.hi, d.at_upper, code, crossed);
        hipLaunchKernelGGL(k_bsens_basic, lp_ceil_div(m, 256), 256, 0, s, d.basis, m, d.lo, d.hi, code, L, H);
        hipLaunchKernelGGL(k_bsens_held, lp_ceil_div(n, 256), 256, 0, s, n, d.lo, d.hi, code, v);
        hipLaunchKernelGGL(k_bsens_bprime, lp_ceil_div(m, 64), 64, 0, s, d.A, m, n, d.b, v, bp);
        hipLaunchKernelGGL(k_bsens_gather, m + 1, 256, 0, s, sd, d.A, bp, d.basis);
        e = hipMemcpyAsync(&hcrossed, crossed, sizeof(int), hipMemcpyDeviceToHost, s);   // read after the crash's sync
    }
    if (e != hipSuccess) rc = -(int)e;
    if (rc == LP_OPTIMAL) rc = lp_simplex_crash(&q);   // m launch pairs, the verdict, rows into position order; one host sync
    if (rc >= 0 && hcrossed) rc = LP_INFEASIBLE;        // the reference checks the bounds before it pivots
    if (rc == LP_OPTIMAL) rc = lp_basis_duals_device(ctx, d.A, m, n, d.b, d.c, d.basis, dy, dd, dw);
    if (rc == LP_OPTIMAL) {
        if (ranging) {
            lp_binv_times_a_launch(ctx, sd, d.A, n, alpha);
            hipLaunchKernelGGL(k_bsens_rhs_ranging, lp_ceil_div(m, 64), dim3(64, 4), 0, s, sd, d.b, d.basis, L, H,
                               d.eps, d.rhs, d.rhs_var, d.rhs_side);
            hipLaunchKernelGGL(k_bsens_cost_ranging, m + lp_ceil_div(n, 256), 256, 0, s, alpha, m, n, d.c, dd, d.basis,
                               code, d.maximize, d.eps, d.cost, d.cost_var);
        } else {
            hipLaunchKernelGGL(k_bsens_x, lp_ceil_div(n, 256), 256, 0, s, sd, n, d.basis, code, v, d.x);
            hipLaunchKernelGGL(k_bsens_w, 1, 256, 0, s, n, dd, v, dw);
        }
        e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->last_error = std::string("bounded basis analysis: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(arena);
    return rc;
}
