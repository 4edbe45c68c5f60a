// batched_lds_loop.hpp — the Gauss-Jordan pivot and the primal simplex loop of the one-LP-per-workgroup kernels
// whose tableau lives in LDS (batched_two_phase.hip, batched_resolve.hip), included INSIDE each kernel after it
// has defined constexpr bool BLAND and the LDS carve (T, pitch, W, prow, lcol, slotvar, basis, pub), m, n, eps,
// tid, wave, lane and d.max_iter.  Not a standalone header.  Shared by inclusion rather than through an inlined
// __device__ function, which changed the register allocation of the existing kernels (batched_two_phase_body.hpp).
// Under the macro LP_BATCHED_DEVEX (k_batched_two_phase_devex only, with BLAND = false and the carve's wts, one
// double per slot) simplex() sets the weights to 1.0 when it starts, prices on d * d / w and updates the weights
// after the ratio test; pivot() — and so the drive-out — never touches them.
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
#ifdef LP_BATCHED_DEVEX
        for (int s = tid; s < n; s += NT) wts[s] = 1.0;
        __syncthreads();
#endif
        for (;;) {
#ifdef LP_BATCHED_DEVEX
            if (wave == 0) {   // the eligible slot of largest score d * d / w, ties to the smallest variable index
                const double* drow = T + (size_t)m * pitch;
                const int se0 = wave_argmax_keyed(n, [&](int s, double& v, int& k, bool& ok) {
                    const double dj = drow[s];
                    v = (dj * dj) / wts[s];
                    k = slotvar[s];
                    ok = (!phase2 || k < n) && (maximize ? (dj > eps) : (dj < -eps));
                });
                if (lane == 0) pub[0] = se0;
            } else
#endif
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
#ifdef LP_BATCHED_DEVEX
                if (r >= 0) {   // weights from the old row r, the old pivot element and the entering slot's old weight;
                                // slot se will hold the leaving variable
                    const double ur = T[(size_t)r * pitch + se], we = wts[se];
                    for (int s = lane; s < n; s += 64)
                        if (s != se) {
                            const double t = T[(size_t)r * pitch + s] / ur;
                            wts[s] = fmax(wts[s], (t * t) * we);
                        }
                    if (lane == 0) wts[se] = fmax(we / (ur * ur), 1.0);
                }
#endif
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
