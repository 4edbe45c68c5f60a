// batched_simplex_body.hpp — the body of the LDS-form batched kernel (batched_simplex.hip), included
// INSIDE the kernels k_batched_simplex<STAMPS> (BLAND = false) and k_batched_simplex_bland (BLAND = true),
// which define the constexpr bools STAMPS and BLAND first.  Not a standalone header.  The body is shared
// by inclusion rather than through an inlined __device__ function because that form changed the register
// allocation of the existing instantiations; included, their device code stays exactly what it was.
// k_batched_simplex_devex defines the macro LP_BATCHED_DEVEX around the inclusion (with BLAND = false): the
// lines under it add the Devex weights (one per slot, behind the carve), their update and the pricing on
// scores; no other kernel sees them.
    extern __shared__ __attribute__((aligned(16))) double smem[];
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev = STAMPS ? __builtin_readcyclecounter() : 0;
#define BS_STAMP(s)                                                          \
    do {                                                                     \
        if (STAMPS) {                                                        \
            const unsigned long long now_ = __builtin_readcyclecounter();    \
            acc[(s)] += now_ - tprev;                                        \
            tprev = now_;                                                    \
        }                                                                    \
    } while (0)
    const int m = d.m, n = d.n, nn = n - m, W = nn + 1, pitch = d.pitch;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lp = blockIdx.x;
    // ---- LDS carve
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = smem + sizeof(Published) / 8;         // (m+1) x pitch
    double* prow = T + (size_t)(m + 1) * pitch;       // W
    double* lcol = prow + W;                          // m+1
    double* ratio = lcol + (m + 1);                   // m
    int* slotvar = reinterpret_cast<int*>(ratio + m); // nn : variable held by each slot
    int* basis = slotvar + nn;                        // m  : N by position
    int* posofvar = basis + m;                        // n  : scratch for the initial split
#ifdef LP_BATCHED_DEVEX
    double* wts = reinterpret_cast<double*>(posofvar + n);   // nn : Devex weight of each slot's variable (2n ints in front)
    for (int s = tid; s < nn; s += nt) wts[s] = 1.0;
#endif

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const int* bin = d.basis_in + (size_t)lp * m;

    // ---- initial condensed tableau for the slack identity basis (Symmetrical.cpp:169-188)
    for (int j = tid; j < n; j += nt) posofvar[j] = -1;
    __syncthreads();
    for (int t = tid; t < m; t += nt) {
        basis[t] = bin[t];
        posofvar[bin[t]] = t;
    }
    __syncthreads();
    if (tid == 0) {  // slots take the non-basic variables in ascending order
        int s = 0;
        for (int j = 0; j < n; ++j)
            if (posofvar[j] < 0) slotvar[s++] = j;
    }
    __syncthreads();
    for (int idx = tid; idx < nn * m; idx += nt) {
        const int s = idx / m, i = idx - s * m;
        T[(size_t)i * pitch + s] = A[(size_t)slotvar[s] * m + i];
    }
    for (int i = tid; i < m; i += nt) T[(size_t)i * pitch + nn] = b[i];
    for (int s = tid; s < nn; s += nt) T[(size_t)m * pitch + s] = c[slotvar[s]];
    if (tid == 0) T[(size_t)m * pitch + nn] = 0.0;
    __syncthreads();

    const double eps = d.eps;
    int iters = 0;
    int status = kRunning;
    const int wave = tid >> 6, lane = tid & 63;
    int* pub = pubs->v;   // [0] entering slot, [1] leaving position, published by wave 0
    // Pricing over the non-basic slots, keyed by variable index (:152-174): wave 0 alone.  It runs
    // for pivot k+1 WHILE the other waves apply pivot k's update to the constraint rows: wave 0
    // updates the reduced-cost row first, which is all the pricing reads.
    auto price = [&]() {
#ifdef LP_BATCHED_DEVEX
        {   // the eligible slot of largest score d * d / w, ties to the smallest variable index
            const double* drow = T + (size_t)m * pitch;
            const int se0 = wave_argmax_keyed(nn, [&](int s, double& v, int& k, bool& ok) {
                const double dj = drow[s];
                v = (dj * dj) / wts[s];
                k = slotvar[s];
                ok = d.maximize ? (dj > eps) : (dj < -eps);
            });
            if (lane == 0) pub[0] = se0;
            return;
        }
#endif
        if constexpr (BLAND) {
            const double* drow = T + (size_t)m * pitch;
            const int se0 = wave_min_key(nn, [&](int s, int& k, bool& ok) {
                const double v = drow[s];
                k = slotvar[s];
                ok = d.maximize ? (v > eps) : (v < -eps);
            });
            if (lane == 0) pub[0] = se0;
            return;
        }
        double best;
        const double* drow = T + (size_t)m * pitch;
        auto getd = [&](int s, double& v, int& k, bool& ok) {
            v = drow[s];
            k = slotvar[s];
            ok = true;
        };
        int se0 = d.maximize ? wave_scan_keyed<true>(nn, eps, best, getd)
                             : wave_scan_keyed<false>(nn, eps, best, getd);
        const bool optimal = d.maximize ? (best <= eps) : (best >= -eps);
        if (optimal) se0 = -1;
        if (lane == 0) pub[0] = se0;
    };
    // the waves other than wave 0 update the constraint rows: ugroups threads per column
    const int unt = nt - 64, ut = tid - 64;
    const int ugroups = unt / W > 0 ? unt / W : 1;
    if (wave == 0) price();
    if (STAMPS) tprev = __builtin_readcyclecounter();
    while (true) {
        BS_STAMP(0);       // wave 0: reduced-cost row + pricing; others: rank-1 update
        __syncthreads();   // tableau complete, pub[0] published
        BS_STAMP(1);       // barrier wait
        if (iters >= d.max_iter) {  // SimplexSolover.h:429,:450
            status = LP_ITER_LIMIT;
            break;
        }
        const int se = pub[0];
        if (se < 0) {
            status = LP_OPTIMAL;
            break;
        }
        // ---- entering column, unbounded test (:176-179), ratios (:185-186) and the ratio test
        // keyed by basis position (:181-194; +inf entries are never taken): wave 0 alone (computing
        // the ratios with all threads first and scanning an LDS array was measured slower: one more
        // barrier than the divisions cost)
        if (wave == 0 && BLAND) {
            int any_pos = 0;
            for (int i = lane; i < m; i += 64)
                if (!(T[(size_t)i * pitch + se] <= eps)) any_pos = 1;
            int r = wave_bland_ratio(m, eps, [&](int i, double& v, int& k) {
                const double ui = T[(size_t)i * pitch + se];
                v = (ui > eps) ? T[(size_t)i * pitch + nn] / ui : NAN;
                k = basis[i];
            });
            if (!__any(any_pos)) r = -1;
            if (lane == 0) pub[1] = r;
        } else if (wave == 0) {
            int r;
            if (m <= 256) {
                // up to four rows per lane: ratios computed once, kept in registers
                double rv[4];
                int any_pos = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = lane + 64 * k;
                    const double ui = (i < m) ? T[(size_t)i * pitch + se] : 0.0;
                    rv[k] = (i < m && ui > eps) ? T[(size_t)i * pitch + nn] / ui : INFINITY;
                    if (i < m && !(ui <= eps)) any_pos = 1;
                }
                r = wave_ratio_select<4>(rv, m, eps);
                if (!__any(any_pos)) r = -1;
            } else {
                int any_pos = 0;
                for (int i = lane; i < m; i += 64)
                    if (!(T[(size_t)i * pitch + se] <= eps)) any_pos = 1;
                double theta;
                auto getr = [&](int i, double& v, int& k, bool& ok) {
                    const double ui = T[(size_t)i * pitch + se];
                    v = (ui > eps) ? T[(size_t)i * pitch + nn] / ui : INFINITY;
                    k = i;
                    ok = true;
                };
                r = wave_scan_keyed<false>(m, eps, theta, getr);
                if (!__any(any_pos)) r = -1;
            }
            if (lane == 0) pub[1] = r;
        }
        BS_STAMP(2);       // wave 0: entering column, ratios, ratio test
        __syncthreads();
        BS_STAMP(3);       // barrier wait (the other waves wait here for the ratio test)
        const int r = pub[1];
        if (r < 0) {
            status = LP_UNBOUNDED;
            break;
        }
        // ---- eta column (:198-204) and a copy of the pivot row
        const double ur = T[(size_t)r * pitch + se];
        const double inv = 1.0 / ur;
        for (int j = tid; j < W; j += nt) prow[j] = T[(size_t)r * pitch + j];
        for (int i = tid; i <= m; i += nt)
            lcol[i] = (i == r) ? inv : -T[(size_t)i * pitch + se] / ur;
        BS_STAMP(4);       // eta column + pivot-row copy
        __syncthreads();
        BS_STAMP(5);       // barrier wait
        // ---- rank-1 update of every stored element; slot se receives the leaving column
        if (wave == 0) {
            // the reduced-cost row, the basis bookkeeping, then the next pivot's pricing
            const double lm = lcol[m];
            double* drow = T + (size_t)m * pitch;
            for (int j = lane; j < W; j += 64) drow[j] = (j == se) ? lm : fma(lm, prow[j], drow[j]);
#ifdef LP_BATCHED_DEVEX
            {   // weights from the old pivot row, the old pivot element and the entering slot's old weight;
                // slot se takes the leaving variable's weight together with its column
                const double we = wts[se];
                for (int j = lane; j < nn; j += 64)
                    if (j != se) {
                        const double t = prow[j] / ur;
                        wts[j] = fmax(wts[j], (t * t) * we);
                    }
                if (lane == 0) wts[se] = fmax(we / (ur * ur), 1.0);
            }
#endif
            if (lane == 0) {
                const int ve = slotvar[se];
                slotvar[se] = basis[r];
                basis[r] = ve;  // N(leave_pos) = enter, :196
            }
            price();
        } else {
            // the constraint rows: a thread owns one column (its pivot-row entry stays in a register)
            // and every ugroups-th row; four rows per step so that their LDS reads are in flight
            // together.  Column se receives the leaving column (the eta column itself).
            for (int slot = ut; slot < ugroups * W; slot += unt) {   // (one slot per thread unless W > unt)
                const int j = slot % W, g = slot / W;
                const double pj = prow[j];
                const bool is_se = (j == se);
                for (int i = g; i < m; i += 4 * ugroups) {
                    double l[4], old[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int iu = i + u * ugroups;
                        const int ic = iu < m ? iu : 0;
                        l[u] = lcol[ic];
                        old[u] = T[(size_t)ic * pitch + j];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int iu = i + u * ugroups;
                        const double t = is_se ? l[u] : (iu == r) ? pj * l[u] : fma(l[u], pj, old[u]);
                        if (iu < m) T[(size_t)iu * pitch + j] = t;
                    }
                }
            }
        }
        ++iters;
    }
    __syncthreads();
    // ---- outputs: x(N(t)) = xB(t), zeros elsewhere (:131-132); basis; counters
    double* x = d.x + (size_t)lp * n;
    for (int j = tid; j < n; j += nt) x[j] = 0.0;
    __syncthreads();
    for (int t = tid; t < m; t += nt) {
        x[basis[t]] = T[(size_t)t * pitch + nn];
        d.basis_out[(size_t)lp * m + t] = basis[t];
    }
    if (tid == 0) {
        d.iters[lp] = iters;
        d.status[lp] = status;
    }
    if (STAMPS && d.stamps && lp == 0 && (tid == 0 || tid == 64)) {
        for (int q = 0; q < 6; ++q) d.stamps[(tid ? 8 : 0) + q] = acc[q];
        d.stamps[(tid ? 8 : 0) + 6] = (unsigned long long)iters;
    }
#undef BS_STAMP
