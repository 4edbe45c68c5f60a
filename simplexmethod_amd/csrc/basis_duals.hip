// basis_duals.hip — the dual solution at a given basis: shadow prices y, reduced costs d and the dual
// objective w = b^T y, exactly as tests/ref/duals_ref.c states them:
//   - T = [B^T | c_B] (m x (m+1)): row t is column basis[t] of A followed by c[basis[t]];
//   - orc_simplex_tableau's crash on the identity basis 0..m-1: step t pivots column t on the unused row of
//     first-max |T[i][t]|, the singular verdict minp <= DBL_EPSILON*m*maxp; y[t] = T[rowpos[t]][m];
//   - d[j] = c[j] - sum_i A[i][j] y[i], one fma chain per column in row order; basic columns exactly 0.0;
//   - w = b^T y, one fma chain in row order.
//
// k_batched_duals: one LP per workgroup, T in LDS (odd row pitch).  Wave 0 selects the pivot row and stages its
// eta column and the pivot row; then every thread applies the rank-1 update to the columns right of the pivot
// column (the columns left of it are unit vectors already and feed nothing the result reads).  The reduced costs
// then read A once, in tiles of 16 rows x NT columns staged through the LDS T held (coalesced along A's columns),
// one column per thread.  Shapes beyond lp_basis_duals_fits: the single-LP launch pair (k_crash_select +
// k_simplex_update, simplex_launch.hip) on an internal (m+1) x ld tableau, then k_reduced_costs.
#include <cfloat>

#include "batched_problem.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kTileRows = 16;   // rows of A per staged tile of the reduced-cost pass

__host__ __device__ inline int duals_threads(int m) { return m <= 64 ? 256 : 512; }
__host__ __device__ inline int duals_pitch(int m) { return (m + 1) | 1; }
// doubles of the region that holds T during the crash, the A tiles and one chunk's basic flags afterwards
__host__ __device__ inline size_t duals_region(int m, int nt) {
    const size_t t = (size_t)m * duals_pitch(m), tiles = (size_t)nt * (kTileRows + 1) + (size_t)nt / 2;
    return t > tiles ? t : tiles;
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_duals(BasisDualsDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int m = d.m, n = d.n, pitch = duals_pitch(m);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve
    int* pub = reinterpret_cast<int*>(smem);               // [0] pivot row, [1] singular verdict, [2] block_any
    double* T = smem + 2;                                  // m x pitch, later the A tiles and the basic flags
    double* yv = T + duals_region(m, NT);                  // m
    double* lcol = yv + m;                                 // m: eta column (entry p = 1/u)
    double* prow = lcol + m;                               // m + 1: pivot row right of the pivot column
    int* rowpos = reinterpret_cast<int*>(prow + m + 1);    // m
    int* used = rowpos + m;                                // m

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const int* N = d.basis + (size_t)lp * m;
    double* y = d.y + (size_t)lp * m;
    double* dd = d.d + (size_t)lp * n;
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
        // ---- T = [B^T | c_B]: row t = column N[t] of A (contiguous: coalesced along i)
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m;
            T[(size_t)t * pitch + i] = A[(size_t)N[t] * m + i];
        }
        for (int t = tid; t < m; t += NT) {
            T[(size_t)t * pitch + m] = c[N[t]];
            used[t] = 0;
        }
        __syncthreads();
        // ---- the crash: wave 0 selects row p and stages lcol / prow; then all threads update columns t+1..m
        double minp = INFINITY, maxp = 0.0;   // wave 0's, wave-uniform
        for (int t = 0; t < m; ++t) {
            if (wave == 0) {
                double big = -1.0;
                int pi = INT_MAX;
                for (int i = lane; i < m; i += 64) {
                    if (used[i]) continue;
                    const double a = fabs(T[(size_t)i * pitch + t]);
                    if (a > big) {   // i ascending per lane: strict > keeps the first maximum
                        big = a;
                        pi = i;
                    }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const double ob = __shfl_xor(big, off, 64);
                    const int op = __shfl_xor(pi, off, 64);
                    if (ob > big || (ob == big && op < pi)) {
                        big = ob;
                        pi = op;
                    }
                }
                int p = -1;
                if (big > 0.0) {
                    p = pi;
                    if (big < minp) minp = big;
                    if (big > maxp) maxp = big;
                    const double u = T[(size_t)p * pitch + t];
                    for (int i = lane; i < m; i += 64)
                        lcol[i] = (i == p) ? 1.0 / u : -T[(size_t)i * pitch + t] / u;
                    for (int j = t + 1 + lane; j <= m; j += 64) prow[j] = T[(size_t)p * pitch + j];
                    if (lane == 0) {
                        used[p] = 1;
                        rowpos[t] = p;
                    }
                }
                if (lane == 0) pub[0] = p;
            }
            __syncthreads();
            const int p = pub[0];
            if (p < 0) {
                status = LP_SINGULAR;
                break;
            }
            // rank-1 update of columns t+1..m (row-major walk: consecutive threads, consecutive columns)
            const int C = m - t;
            const int qs = NT / C, rs = NT - qs * C;
            int i = tid / C, jj = tid - i * C;
            for (int e = tid; e < m * C; e += NT) {
                const int j = t + 1 + jj;
                double* Tij = T + (size_t)i * pitch + j;
                *Tij = (i == p) ? prow[j] * lcol[i] : fma(lcol[i], prow[j], *Tij);
                i += qs;
                jj += rs;
                if (jj >= C) {
                    jj -= C;
                    ++i;
                }
            }
            for (int i = tid; i < m; i += NT) T[(size_t)i * pitch + t] = (i == p) ? 1.0 : 0.0;
            __syncthreads();
        }
        if (status == LP_OPTIMAL) {
            if (tid == 0) pub[1] = minp <= DBL_EPSILON * (double)m * maxp;
            __syncthreads();
            if (pub[1]) status = LP_SINGULAR;
        }
    }
    if (status != LP_OPTIMAL) {
        for (int t = tid; t < m; t += NT) y[t] = NAN;
        for (int j = tid; j < n; j += NT) dd[j] = NAN;
        if (tid == 0) {
            d.w[lp] = NAN;
            d.status[lp] = status;
        }
        return;
    }
    for (int t = tid; t < m; t += NT) {
        const double v = T[(size_t)rowpos[t] * pitch + m];
        yv[t] = v;
        y[t] = v;
    }
    __syncthreads();   // T is free: it holds the A tiles from here on
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = fma(b[i], yv[i], s);
        d.w[lp] = s;
        d.status[lp] = LP_OPTIMAL;
    }
    double* tile = T;   // NT columns x kTileRows rows, column pitch kTileRows + 1 (odd)
    int* basic = reinterpret_cast<int*>(T + (size_t)NT * (kTileRows + 1));   // NT: one column chunk's basic flags
    for (int j0 = 0; j0 < n; j0 += NT) {
        basic[tid] = 0;
        __syncthreads();
        for (int t = tid; t < m; t += NT)
            if (N[t] >= j0 && N[t] < j0 + NT) basic[N[t] - j0] = 1;
        const int j = j0 + tid;
        double s = j < n ? c[j] : 0.0;
        for (int i0 = 0; i0 < m; i0 += kTileRows) {
            const int rows = m - i0 < kTileRows ? m - i0 : kTileRows;
            for (int e = tid; e < NT * kTileRows; e += NT) {
                const int cc = e / kTileRows, rr = e % kTileRows;
                if (rr < rows && j0 + cc < n) tile[cc * (kTileRows + 1) + rr] = A[(size_t)(j0 + cc) * m + i0 + rr];
            }
            __syncthreads();
            if (j < n)
                for (int rr = 0; rr < rows; ++rr) s = fma(-tile[tid * (kTileRows + 1) + rr], yv[i0 + rr], s);
            __syncthreads();
        }
        if (j < n) dd[j] = basic[tid] ? 0.0 : s;
    }
}

template <int NT>
int batched_duals_launch(lp_context* ctx, const BasisDualsDev& d) {
    return lp_launch_per_lp(ctx, k_batched_duals<NT>, NT, lp_basis_duals_lds_bytes(d.m), d);
}

// ---- the single-LP path beyond lp_basis_duals_fits

// T (m+1 rows, pitch ld) = [B^T | c_B; 0]; the crash bookkeeping's basis = 0..m-1
__global__ __launch_bounds__(256) void k_duals_gather(SimplexDev s, const double* A, const double* c,
                                                      const int* basis) {
    const int t = blockIdx.x;   // tableau row, 0..m
    const int m = s.m;
    double* row = s.T + (size_t)t * s.ld;
    if (t == m) {
        for (int j = threadIdx.x; j < s.ld; j += blockDim.x) row[j] = 0.0;
        return;
    }
    const double* col = A + (size_t)basis[t] * m;
    for (int j = threadIdx.x; j < s.ld; j += blockDim.x)
        row[j] = (j < m) ? col[j] : (j == m) ? c[basis[t]] : 0.0;
    if (threadIdx.x == 0) s.basis[t] = t;
}

// y from the crashed tableau (rows in position order), then d (one column per thread) and w (thread 0)
__global__ __launch_bounds__(256) void k_reduced_costs(SimplexDev s, const double* A, const double* b,
                                                       const double* c, int n, double* y, double* dd, double* w) {
    const int m = s.m;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) {
        double v = c[j];
        const double* a = A + (size_t)j * m;
        for (int i = 0; i < m; ++i) v = fma(-a[i], s.T[(size_t)i * s.ld + m], v);
        dd[j] = v;
    }
    if (j < m) y[j] = s.T[(size_t)j * s.ld + m];
    if (j == 0) {
        double v = 0.0;
        for (int i = 0; i < m; ++i) v = fma(b[i], s.T[(size_t)i * s.ld + m], v);
        *w = v;
    }
}

__global__ __launch_bounds__(256) void k_zero_basic(const int* basis, int m, double* dd) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) dd[basis[t]] = 0.0;
}

}  // namespace

size_t lp_basis_duals_lds_bytes(int m) {
    const int nt = duals_threads(m);
    // pub (2 doubles), the region, yv + lcol + prow, rowpos + used
    return sizeof(double) * (2 + duals_region(m, nt) + 3 * (size_t)m + 1) + sizeof(int) * 2 * (size_t)m;
}

int lp_basis_duals_launch(lp_context* ctx, const BasisDualsDev& d) {
    if (!lp_basis_duals_fits(d.m)) LP_FAIL(ctx, LP_BAD_ARG, "basis duals: m does not fit one CU's LDS");
    if (d.batch <= 0) return LP_OPTIMAL;
    if (duals_threads(d.m) == 256) return batched_duals_launch<256>(ctx, d);
    return batched_duals_launch<512>(ctx, d);
}

// One LP of any size on the device: A, b, c, basis already there (basis range checked by the caller).
int lp_basis_duals_device(lp_context* ctx, const double* dA, int m, int n, const double* db, const double* dc,
                          const int* dbasis, double* dy, double* dd, double* dw) {
    hipStream_t s = ctx->stream;
    const int ld = (int)lp_ceil_div<size_t>((size_t)m + 1, 8) * 8;
    lp_simplex_problem q;
    q.ctx = ctx;
    q.tableau_bytes = sizeof(double) * (size_t)(m + 1) * ld;
    SimplexDev& sd = q.dev;
    sd.m = m;
    sd.n = m;   // the right-hand-side column of [B^T | c_B]
    sd.ld = ld;
    // one allocation: T, the pristine copy the crash permutes through, lcol, prow, state, basis, rowpos, rowused
    auto pieces = [&](lp_carver& cv) {
        sd.T = cv.take<double>(q.tableau_bytes);
        q.dT0 = cv.take<double>(q.tableau_bytes);
        sd.lcol = cv.take<double>(sizeof(double) * ((size_t)m + 1));
        sd.prow = cv.take<double>(sizeof(double) * (size_t)ld);
        sd.state = cv.take<SimplexState>(sizeof(SimplexState));
        sd.basis = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowpos = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowused = cv.take<unsigned char>((size_t)m);
    };
    char* arena = nullptr;
    LP_HIP(ctx, lp_carve_malloc(&arena, pieces));
    hipLaunchKernelGGL(k_duals_gather, m + 1, 256, 0, s, sd, dA, dc, dbasis);
    int rc = lp_simplex_crash(&q);   // m launch pairs, the verdict, rows into position order; one host sync
    if (rc == LP_OPTIMAL) {
        hipLaunchKernelGGL(k_reduced_costs, lp_ceil_div(n > m ? n : m, 256), 256, 0, s, sd, dA, db, dc, n, dy, dd,
                           dw);
        hipLaunchKernelGGL(k_zero_basic, lp_ceil_div(m, 256), 256, 0, s, dbasis, m, dd);
        hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->last_error = std::string("basis duals: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(arena);
    return rc;
}
