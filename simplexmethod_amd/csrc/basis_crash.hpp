// basis_crash.hpp — device pieces shared by basis_ranging.hip and basis_certificate.hip: the first-index
// (value, index) reductions and the crash on an m x (m+1) tableau (the [B^T | c_B] form, or [B | I | b] kept in
// place).  Each including file gets its own internal copy, so the device code of either kernel depends only on the
// text below.
#pragma once

#include <cfloat>
#include <climits>

#include "lp_internal.hpp"

namespace {

// (v, k) replaces the best (bv, bk) when there is none yet, when it is strictly better (larger for WANT_MAX), or on
// a tie at a smaller index; k < 0 is no candidate.  The side is a template parameter: with a run-time flag selecting
// the comparison, -O3 code for the shuffle reduction below returned wrong winners on gfx950.
template <bool WANT_MAX>
__device__ inline void take(double v, int k, double& bv, int& bk) {
    if (k >= 0 && (bk < 0 || (WANT_MAX ? v > bv : v < bv) || (v == bv && k < bk))) {
        bv = v;
        bk = k;
    }
}

template <bool WANT_MAX>
__device__ inline void wave_take(double& v, int& k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int ok = __shfl_xor(k, off, 64);
        take<WANT_MAX>(ov, ok, v, k);
    }
}

// The crash on the m x (m+1) tableau T (row pitch `pitch`) with the identity basis.  INPLACE = false: [B^T | c_B],
// columns right of the pivot column only (k_batched_duals's update).  INPLACE = true: [B | b] standing for
// [B | I | b], every column but t updated, slot t takes the pivot row's identity column.  Block-uniform status.
template <int NT, bool INPLACE>
__device__ int ranging_crash(double* T, int m, int pitch, double* lcol, double* prow, int* used, int* rowpos,
                             int* zneg, int* pub) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
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
                for (int j = (INPLACE ? 0 : t + 1) + lane; j <= m; j += 64) prow[j] = T[(size_t)p * pitch + j];
                if (lane == 0) {
                    used[p] = 1;
                    rowpos[t] = p;
                }
            }
            if (lane == 0) pub[0] = p;
        }
        __syncthreads();
        const int p = pub[0];
        if (p < 0) return LP_SINGULAR;
        // rank-1 update (row-major walk: consecutive threads, consecutive columns)
        const int j0 = INPLACE ? 0 : t + 1;
        const int C = m + 1 - j0;
        const int qs = NT / C, rs = NT - qs * C;
        int i = tid / C, jj = tid - i * C;
        for (int e = tid; e < m * C; e += NT) {
            const int j = j0 + jj;
            double* Tij = T + (size_t)i * pitch + j;
            if (!INPLACE || j != t) {
                *Tij = (i == p) ? prow[j] * lcol[i] : fma(lcol[i], prow[j], *Tij);
            } else {   // identity column m+p: 1.0 in row p, the implicit zero elsewhere
                const double z = zneg[i] ? -0.0 : 0.0;
                *Tij = (i == p) ? 1.0 * lcol[i] : fma(lcol[i], 1.0, z);
                if (i == p) zneg[i] = signbit(lcol[i]) ? 1 : 0;   // +0.0 * (1/u)
                else if (used[i]) zneg[i] = zneg[i] && signbit(lcol[i]);   // fma(l, +0.0, z)
            }
            i += qs;
            jj += rs;
            if (jj >= C) {
                jj -= C;
                ++i;
            }
        }
        __syncthreads();
    }
    if (tid == 0) pub[1] = minp <= DBL_EPSILON * (double)m * maxp;
    __syncthreads();
    return pub[1] ? LP_SINGULAR : LP_OPTIMAL;
}

}  // namespace
