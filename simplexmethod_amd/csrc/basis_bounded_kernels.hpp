// basis_bounded_kernels.hpp — the small kernels that the single-LP paths of basis_bounded.hip (lp_basis_bounded_device)
// and basis_bounded_certificate.hip (lp_basis_bounded_certificate_device) share: the column codes with the
// crossed-bound word, the held values, and one fma chain per row against a held vector (b', and the certificate's b0).
// Each including file gets its own internal copy, so the device code of either path depends only on the text below.
#pragma once

#include "lp_internal.hpp"

namespace {

enum { kLower = 0, kBasic = 1, kUpper = 2 };   // what code[j] says of column j

// code[j] by the flag alone (the per-position kernel overwrites the basic columns'); any hi_j < lo_j raises *crossed
__global__ __launch_bounds__(256) void k_bsens_codes(int n, const double* lo, const double* hi, const int* up,
                                                     int* code, int* crossed) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    code[j] = up[j] ? kUpper : kLower;
    if (hi[j] < lo[j]) *crossed = 1;
}

// the held values: 0.0 for basic columns
__global__ __launch_bounds__(256) void k_bsens_held(int n, const double* lo, const double* hi, const int* code,
                                                    double* v) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) v[j] = code[j] == kBasic ? 0.0 : code[j] == kUpper ? hi[j] : lo[j];
}

// b'[i] = b[i] - sum_j A[i][j] v_j: one chain per row (one thread), j ascending over v_j != 0.0; consecutive threads
// read consecutive i of column j, and v_j is the same for the whole block
__global__ __launch_bounds__(64) void k_bsens_bprime(const double* A, int m, int n, const double* b, const double* v,
                                                     double* bp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double acc = b[i];
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const double vj = v[j];
        if (vj != 0.0) acc = fma(-A[(size_t)j * m + i], vj, acc);
    }
    bp[i] = acc;
}

}  // namespace
