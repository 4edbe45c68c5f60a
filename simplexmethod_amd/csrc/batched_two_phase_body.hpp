// batched_two_phase_body.hpp — the body of the batched two-phase kernel (batched_two_phase.hip), included
// INSIDE the kernels k_batched_two_phase<NT> (BLAND = false) and k_batched_two_phase_bland<NT> (BLAND =
// true), which define the constexpr bool BLAND first.  Not a standalone header.  The body is shared by
// inclusion rather than through an inlined __device__ function because that form changed the register
// allocation of the existing instantiations; included, their device code stays exactly what it was.
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

    // ---- one Gauss-Jordan pivot on (row r, slot se) with tableau_pivot's arithmetic; slot se
    // receives the leaving variable's column (the eta column itself).  All threads.
    const int G = NT / W > 0 ? NT / W : 1;   // row groups: a thread owns one column and every G-th row
    auto pivot = [&](int r, int se) {
        const double ur = T[(size_t)r * pitch + se];
        for (int j = tid; j < W; j += NT) prow[j] = T[(size_t)r * pitch + j];
        for (int i = tid; i <= m; i += NT) lcol[i] = (i == r) ? 1.0 / ur : -T[(size_t)i * pitch + se] / ur;
        __syncthreads();
        for (int slot = tid; slot < G * W; slot += NT) {
            const int j = slot % W, g = slot / W;
            const double pj = prow[j];
            for (int i = g; i <= m; i += G) {
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

    // ---- tableau_loop: pricing keyed by variable index over the eligible slots, ratio test keyed by
    // basis position, both by wave 0.  Phase II bars the artificial slots.
    auto simplex = [&](bool phase2, bool maximize, int& iters) -> int {
        if (d.max_iter <= 0) return LP_ITER_LIMIT;
        for (;;) {
            if (wave == 0 && BLAND) {
                const double* drow = T + (size_t)m * pitch;
                const int se0 = wave_min_key(n, [&](int s, int& k, bool& ok) {
                    const double v = drow[s];
                    k = slotvar[s];
                    ok = (!phase2 || k < n) && (maximize ? (v > eps) : (v < -eps));
                });
                if (lane == 0) pub[0] = se0;
            } else if (wave == 0) {
                double best;
                const double* drow = T + (size_t)m * pitch;
                auto getd = [&](int s, double& v, int& k, bool& ok) {
                    v = drow[s];
                    k = slotvar[s];
                    ok = !phase2 || k < n;
                };
                int se0 = maximize ? wave_scan_keyed<true>(n, eps, best, getd)
                                   : wave_scan_keyed<false>(n, eps, best, getd);
                const bool optimal = maximize ? (best <= eps) : (best >= -eps);
                if (lane == 0) pub[0] = optimal ? -1 : se0;
            }
            __syncthreads();
            const int se = pub[0];
            if (se < 0) return LP_OPTIMAL;
            if (wave == 0 && BLAND) {
                int any_pos = 0;
                for (int i = lane; i < m; i += 64)
                    if (!(T[(size_t)i * pitch + se] <= eps)) any_pos = 1;
                int r = wave_bland_ratio(m, eps, [&](int i, double& v, int& k) {
                    const double ui = T[(size_t)i * pitch + se];
                    v = (ui > eps) ? T[(size_t)i * pitch + n] / ui : NAN;
                    k = basis[i];
                });
                if (!__any(any_pos)) r = -1;
                if (lane == 0) pub[1] = r;
            } else if (wave == 0) {
                int r, any_pos = 0;
                if (m <= 128) {
                    double rv[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int i = lane + 64 * k;
                        const double ui = (i < m) ? T[(size_t)i * pitch + se] : 0.0;
                        rv[k] = (i < m && ui > eps) ? T[(size_t)i * pitch + n] / ui : INFINITY;
                        if (i < m && !(ui <= eps)) any_pos = 1;
                    }
                    r = wave_ratio_select<2>(rv, m, eps);
                } else if (m <= 256) {
                    double rv[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int i = lane + 64 * k;
                        const double ui = (i < m) ? T[(size_t)i * pitch + se] : 0.0;
                        rv[k] = (i < m && ui > eps) ? T[(size_t)i * pitch + n] / ui : INFINITY;
                        if (i < m && !(ui <= eps)) any_pos = 1;
                    }
                    r = wave_ratio_select<4>(rv, m, eps);
                } else {
                    for (int i = lane; i < m; i += 64)
                        if (!(T[(size_t)i * pitch + se] <= eps)) any_pos = 1;
                    double theta;
                    auto getr = [&](int i, double& v, int& k, bool& ok) {
                        const double ui = T[(size_t)i * pitch + se];
                        v = (ui > eps) ? T[(size_t)i * pitch + n] / ui : INFINITY;
                        k = i;
                        ok = true;
                    };
                    r = wave_scan_keyed<false>(m, eps, theta, getr);
                }
                if (!__any(any_pos)) r = -1;
                if (lane == 0) pub[1] = r;
            }
            __syncthreads();
            const int r = pub[1];
            if (r < 0) return LP_UNBOUNDED;
            pivot(r, se);
            ++iters;
            if (iters >= d.max_iter) return LP_ITER_LIMIT;
        }
    };

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
