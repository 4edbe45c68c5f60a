// basis_col_chains.hpp — the staged-tile column chains shared by basis_certificate.hip and
// basis_bounded_certificate.hip: R weight rows against a chunk of kCW columns of A, one column per thread, A staged
// through LDS in tiles of kTR rows.  Each including file gets its own internal copy, so the device code of either
// kernel depends only on the text below.
#pragma once

#include "lp_internal.hpp"

namespace {

constexpr int kCW = 256;   // columns per chunk of the alpha passes (one per thread of the first group)
constexpr int kTR = 8;     // rows of A per staged tile

// acc[r] = sum_i W[rp[r] + (slot ? slot[i] : i)] * A[i][j0 + tid] for tid < kCW, the chain fma(w, a, acc) over i
// ascending from 0; A staged through `tile` (column pitch kTR + 1).  Every thread of the block calls it.
template <int NT, int R>
__device__ inline void col_chains(const double* A, int m, int n, int j0, double* tile, const double* W,
                                  const int (&rp)[R], const int* slot, double (&acc)[R]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    for (int i0 = 0; i0 < m; i0 += kTR) {
        const int rows = m - i0 < kTR ? m - i0 : kTR;
        __syncthreads();   // the tile's previous readers are done
        for (int e = tid; e < kCW * kTR; e += NT) {
            const int cc = e / kTR, rr = e % kTR;
            if (rr < rows && j0 + cc < n) tile[cc * (kTR + 1) + rr] = A[(size_t)(j0 + cc) * m + i0 + rr];
        }
        __syncthreads();
        if (tid < kCW && j0 + tid < n)
            for (int rr = 0; rr < rows; ++rr) {
                const double a = tile[tid * (kTR + 1) + rr];
                const int k = slot ? slot[i0 + rr] : i0 + rr;
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fma(W[rp[r] + k], a, acc[r]);
            }
    }
    __syncthreads();
}

}  // namespace
