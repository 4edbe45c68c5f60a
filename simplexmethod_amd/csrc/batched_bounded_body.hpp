// batched_bounded_body.hpp — the body of k_batched_bounded<NT> and of its rule forms (batched_bounded.hip, which
// describes the flow and the layout), included INSIDE each of them. As it stands it runs Dantzig's rule; under the
// macro LP_BOUNDED_BLAND or LP_BOUNDED_DEVEX batched_bounded_loop.hpp's loop runs that rule, and under
// LP_BOUNDED_DEVEX the carve carries the weights (wts). BLAND = false is for batched_lds_loop.hpp, of which only the
// pivot is used. Not a standalone header.
    constexpr bool BLAND = false;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    char* base = reinterpret_cast<char*>(smem);
    const int m = d.m, n = d.n, W = n + 1;
#ifdef LP_BOUNDED_DEVEX
    const BoundedCarve K = bounded_carve(m, n, true);
#else
    const BoundedCarve K = bounded_carve(m, n);
#endif
    const int pitch = K.pitch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = reinterpret_cast<double*>(base + K.T);
    double* prow = reinterpret_cast<double*>(base + K.prow);
    double* lcol = reinterpret_cast<double*>(base + K.lcol);
    double* U = reinterpret_cast<double*>(base + K.U);
    double* lov = reinterpret_cast<double*>(base + K.lov);
    int* slotvar = reinterpret_cast<int*>(base + K.slotvar);
    int* basis = reinterpret_cast<int*>(base + K.basis);
    int* up = reinterpret_cast<int*>(base + K.up);
#ifdef LP_BOUNDED_DEVEX
    double* wts = reinterpret_cast<double*>(base + K.wts);   // the Devex weights, one per slot
#endif
    int* pub = pubs->v;   // [0] entering slot, [1] leaving position, [2] action / infeasible, [3] hi < lo

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* lo = d.lo + (size_t)lp * n;
    const double* hi = d.hi + (size_t)lp * n;
    const double eps = d.eps;

    // ---- load: slots = original columns in order, basis = the artificials by position, nothing complemented
    for (int s = tid; s < n; s += NT) {
        const double l = lo[s];
        slotvar[s] = s;
        up[s] = 0;
        lov[s] = l;
        U[s] = hi[s] - l;
    }
    for (int t = tid; t < m; t += NT) basis[t] = n + t;
    for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
        const int s = e / m, i = e - s * m;
        T[(size_t)i * pitch + s] = A[e];
    }
    __syncthreads();
    // ---- shift (one chain per row, lo_j == 0 skipped) and the auxiliary problem's sign changes
    for (int i = tid; i < m; i += NT) {
        double acc = b[i];
        for (int j = 0; j < n; ++j) {
            const double l = lov[j];
            if (l != 0.0) acc = fma(-T[(size_t)i * pitch + j], l, acc);
        }
        const bool flip = acc < -eps;
        T[(size_t)i * pitch + n] = flip ? -acc : acc;
        lcol[i] = flip ? -1.0 : 1.0;
    }
    if (wave == 0) {
        int bad = 0;
        for (int s = lane; s < n; s += 64)
            if (U[s] < 0.0) bad = 1;
        bad = __any(bad);
        if (lane == 0) pub[3] = bad;
    }
    __syncthreads();
    const bool crossed = pub[3] != 0;
    if (!crossed) {
        for (int e = tid; e < m * n; e += NT) {
            const int i = e / n, s = e - i * n;
            if (lcol[i] < 0.0) T[(size_t)i * pitch + s] = -T[(size_t)i * pitch + s];
        }
        __syncthreads();
        // ---- phase-I reduced costs: the artificial basis' crash, one serial chain per column
        for (int j = tid; j < W; j += NT) {
            double dj = 0.0;
            for (int t = 0; t < m; ++t) dj = fma(-1.0, T[(size_t)t * pitch + j], dj);
            T[(size_t)m * pitch + j] = dj;
        }
        __syncthreads();
    }

#include "batched_lds_loop.hpp"
#include "batched_bounded_loop.hpp"
    (void)simplex;   // (batched_lds_loop.hpp's unbounded loop: only its pivot is used here)

    int it[4] = {0, 0, 0, 0};
    int status = LP_INFEASIBLE;
    if (!crossed) {
        // ---- phase I: minimise the sum of the artificials; every slot may enter
        status = bounded_simplex(false, false, it[0], it[3]);
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
                const int s0 =
                    kmin == INT_MAX ? -1 : __builtin_amdgcn_readlane(sbest, (int)__builtin_ctzll(__ballot(kbest == kmin)));
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
            // ---- phase-II reduced costs: c' (c_j, or -c_j for a complemented column) priced out over the basis in
            // position order
            auto cost = [&](int k) -> double { return k < n ? (up[k] ? -c[k] : c[k]) : 0.0; };
            for (int t = tid; t < m; t += NT) lcol[t] = -cost(basis[t]) / 1.0;
            __syncthreads();
            for (int j = tid; j < W; j += NT) {
                double dj = j < n ? cost(slotvar[j]) : 0.0;
                for (int t = 0; t < m; ++t) dj = fma(lcol[t], T[(size_t)t * pitch + j], dj);
                T[(size_t)m * pitch + j] = dj;
            }
            __syncthreads();
            // ---- phase II: artificial slots never enter; max_iter counts from 0 again
            status = bounded_simplex(true, d.maximize != 0, it[2], it[3]);
            __syncthreads();
        }
    }
    // ---- outputs: x_j = lo_j + (up_j ? U_j - v_j : v_j) (lo_j == 0: no addition) for LP_OPTIMAL; basis, flags and
    // counters always (an LP with hi < lo: the starting basis, nothing complemented, zero counters)
    if (status == LP_OPTIMAL) {
        for (int j = tid; j < n; j += NT) prow[j] = 0.0;
        __syncthreads();
        for (int t = tid; t < m; t += NT)
            if (basis[t] < n) prow[basis[t]] = T[(size_t)t * pitch + n];
        __syncthreads();
        double* x = d.x + (size_t)lp * n;
        for (int j = tid; j < n; j += NT) {
            const double v = prow[j];
            const double w = up[j] ? U[j] - v : v;
            x[j] = lov[j] == 0.0 ? w : lov[j] + w;
        }
    }
    for (int t = tid; t < m; t += NT) d.basis_out[(size_t)lp * m + t] = basis[t];
    for (int j = tid; j < n; j += NT) d.at_upper[(size_t)lp * n + j] = up[j];
    if (tid == 0) {
        int* io = d.iters + (size_t)lp * 4;
        io[0] = it[0];
        io[1] = it[1];
        io[2] = it[2];
        io[3] = it[3];
        d.status[lp] = status;
    }
