// batched_two_phase_body.hpp — the body of the batched two-phase kernel (batched_two_phase.hip), included
// INSIDE the kernels k_batched_two_phase<NT> (BLAND = false) and k_batched_two_phase_bland<NT> (BLAND =
// true), which define the constexpr bool BLAND first.  Not a standalone header.  The body is shared by
// inclusion rather than through an inlined __device__ function because that form changed the register
// allocation of the existing instantiations; included, their device code stays exactly what it was.
// k_batched_two_phase_devex<NT> defines the macro LP_BATCHED_DEVEX around the inclusion (with BLAND = false):
// the carve then ends with the Devex weights, which batched_lds_loop.hpp's simplex() owns.
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int m = d.m, n = d.n, W = n + 1, pitch = d.pitch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = smem + sizeof(Published) / 8;             // (m+1) x pitch
    double* prow = T + (size_t)(m + 1) * pitch;           // W
    double* lcol = prow + W;                              // m+1
    int* slotvar = reinterpret_cast<int*>(lcol + m + 1);  // n
    int* basis = slotvar + n;                             // m
#ifdef LP_BATCHED_DEVEX
    double* wts = reinterpret_cast<double*>(basis + m + ((n + m) & 1));   // n : Devex weight of each slot's variable
#endif
    int* pub = pubs->v;   // [0] entering slot, [1] leaving position, [2] infeasible: published by wave 0

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double eps = d.eps;

    // ---- auxiliary problem (make_b_nonneg, createAuxiliaryProblem): slots = original columns in
    // order, basis = the artificials by position
    for (int s = tid; s < n; s += NT) slotvar[s] = s;
    for (int t = tid; t < m; t += NT) basis[t] = n + t;
    for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
        const int s = e / m, i = e - s * m;
        const double a = A[e];
        T[(size_t)i * pitch + s] = (b[i] < -eps) ? -a : a;
    }
    for (int i = tid; i < m; i += NT) T[(size_t)i * pitch + n] = (b[i] < -eps) ? -b[i] : b[i];
    __syncthreads();
    // ---- phase-I reduced costs: the artificial basis' crash, one serial chain per column
    for (int j = tid; j < W; j += NT) {
        double dj = 0.0;
        for (int t = 0; t < m; ++t) dj = fma(-1.0, T[(size_t)t * pitch + j], dj);
        T[(size_t)m * pitch + j] = dj;
    }
    __syncthreads();

#include "batched_lds_loop.hpp"

    int it[3] = {0, 0, 0};
    // ---- phase I: minimise the sum of the artificials; every slot may enter
    int status = simplex(false, false, it[0]);
    __syncthreads();
    if (status == LP_OPTIMAL) {
        // the artificials' values by artificial index, summed in that order
        for (int i = tid; i < m; i += NT) lcol[i] = 0.0;
        __syncthreads();
        for (int t = tid; t < m; t += NT)
            if (basis[t] >= n) lcol[basis[t] - n] = T[(size_t)t * pitch + n];
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int i = 0; i < m; ++i) sum += lcol[i];
            pub[2] = sum > eps;
        }
        __syncthreads();
        if (pub[2]) status = LP_INFEASIBLE;
    }
    // ---- drive-out: every position still holding an artificial, in ascending order
    for (int pos = 0; pos < m && status == LP_OPTIMAL; ++pos) {
        if (basis[pos] < n) continue;
        if (wave == 0) {   // the eligible slot of smallest variable index
            int kbest = INT_MAX, sbest = -1;
            for (int s = lane; s < n; s += 64) {
                const int k = slotvar[s];
                if (k < n && k < kbest && fabs(T[(size_t)pos * pitch + s]) > eps) {
                    kbest = k;
                    sbest = s;
                }
            }
            const int kmin = (int)lpdev::wave_ext_u32<false>((unsigned)kbest);
            const int s0 = kmin == INT_MAX ? -1 : __builtin_amdgcn_readlane(sbest, (int)__builtin_ctzll(__ballot(kbest == kmin)));
            if (lane == 0) pub[0] = s0;
        }
        __syncthreads();
        const int s = pub[0];
        if (s < 0) {
            status = LP_SINGULAR;
            break;
        }
        pivot(pos, s);
        ++it[1];
    }
    __syncthreads();
    if (status == LP_OPTIMAL) {
        // ---- phase-II reduced costs: c priced out over the basis in position order
        for (int t = tid; t < m; t += NT) lcol[t] = -c[basis[t]] / 1.0;
        __syncthreads();
        for (int j = tid; j < W; j += NT) {
            double dj = (j < n && slotvar[j] < n) ? c[slotvar[j]] : 0.0;
            for (int t = 0; t < m; ++t) dj = fma(lcol[t], T[(size_t)t * pitch + j], dj);
            T[(size_t)m * pitch + j] = dj;
        }
        __syncthreads();
        // ---- phase II: artificial slots never enter; max_iter counts from 0 again
        status = simplex(true, d.maximize != 0, it[2]);
        __syncthreads();
    }
    // ---- outputs: x(N(t)) = xB(t), zeros elsewhere; basis; counters
    double* x = d.x + (size_t)lp * n;
    for (int j = tid; j < n; j += NT) x[j] = 0.0;
    __syncthreads();
    for (int t = tid; t < m; t += NT) {
        if (basis[t] < n) x[basis[t]] = T[(size_t)t * pitch + n];
        d.basis_out[(size_t)lp * m + t] = basis[t];
    }
    if (tid == 0) {
        d.iters[(size_t)lp * 3 + 0] = it[0];
        d.iters[(size_t)lp * 3 + 1] = it[1];
        d.iters[(size_t)lp * 3 + 2] = it[2];
        d.status[lp] = status;
    }
