// batched_bounded_loop.hpp — the bounded-variable primal simplex loop of batched_bounded.hip: Dantzig pricing as
// batched_lds_loop.hpp, the bounded ratio test, the bound flip and the complement of a variable that leaves at its
// upper bound (tests/ref/bounded_ref.c steps 5-6).  Included INSIDE k_batched_bounded<NT> after batched_lds_loop.hpp
// (whose pivot it uses) and after the kernel has defined the LDS carve (T, pitch, prow, lcol, U, up, slotvar, basis,
// pub), m, n, eps, tid, wave, lane and d.max_iter.  Not a standalone header.
// Under the macro LP_BOUNDED_BLAND (the _bland kernels of batched_bounded.hip and batched_bounded_resolve.hip) the
// loop prices by smallest variable index and runs Bland's bounded ratio test, in which the entering variable's own
// width is one more blocking candidate keyed by its index (batched_scan.hpp: wave_bland_ratio_entering).  Under
// LP_BOUNDED_DEVEX (the _devex kernels, with the carve's wts, one double per slot) it sets the weights to 1.0 when it
// starts, prices on d * d / w and, ahead of a pivot, updates the weights from the row that leaves; the ratio test, the
// flip decision and the complement are Dantzig's, and a flip leaves the weights alone.  Without either macro the
// code is what it was (tests/ref/bounded_rules_ref.c states the three).
    // the width of variable k: hi - lo for a structural, +inf for an artificial
    auto ubound = [&](int k) -> double { return k < n ? U[k] : INFINITY; };

    // One phase: pricing by wave 0 (the variable-keyed chain); the ratio test by wave 0 (the position-keyed chain)
    // with the bounded values, then the action published in pub[2]: -1 unbounded, 1 flip, 0 pivot, 2 complement row
    // pub[1] and pivot.  `pivots` counts this phase's pivots, `flips` every flip; max_iter bounds their sum here.
    auto bounded_simplex = [&](bool phase2, bool maximize, int& pivots, int& flips) -> int {
        if (d.max_iter <= 0) return LP_ITER_LIMIT;
        int count = 0;
#ifdef LP_BOUNDED_DEVEX
        for (int s = tid; s < n; s += NT) wts[s] = 1.0;
        __syncthreads();
#endif
        for (;;) {
#if defined(LP_BOUNDED_DEVEX)
            if (wave == 0) {   // the eligible slot of largest score d * d / w, ties to the smallest variable index
                const double* drow = T + (size_t)m * pitch;
                const int se0 = wave_argmax_keyed(n, [&](int s, double& v, int& k, bool& ok) {
                    const double dj = drow[s];
                    v = (dj * dj) / wts[s];
                    k = slotvar[s];
                    ok = (!phase2 || k < n) && (maximize ? (dj > eps) : (dj < -eps));
                });
                if (lane == 0) pub[0] = se0;
            }
#elif defined(LP_BOUNDED_BLAND)
            if (wave == 0) {   // the eligible slot of smallest variable index
                const double* drow = T + (size_t)m * pitch;
                const int se0 = wave_min_key(n, [&](int s, int& k, bool& ok) {
                    const double v = drow[s];
                    k = slotvar[s];
                    ok = (!phase2 || k < n) && (maximize ? (v > eps) : (v < -eps));
                });
                if (lane == 0) pub[0] = se0;
            }
#else
            if (wave == 0) {
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
#endif
            __syncthreads();
            const int se = pub[0];
            if (se < 0) return LP_OPTIMAL;
#ifdef LP_BOUNDED_BLAND
            if (wave == 0) {
                // Dantzig's bounded row values (NaN: no candidate) keyed by the basic variable, and the entering
                // variable's own width keyed by its index: the smallest key within eps of the exact minimum
                const int e = slotvar[se];
                const int r = wave_bland_ratio_entering(m, eps, ubound(e), e, [&](int i, double& v, int& k) {
                    const double a = T[(size_t)i * pitch + se], xb = T[(size_t)i * pitch + n];
                    const double u = ubound(basis[i]);
                    v = (a > eps) ? xb / a : (a < -eps && u < INFINITY) ? (xb - u) / a : NAN;
                    k = basis[i];
                });
                const int act = (r == -1) ? -1 : (r == -2) ? 1 : (T[(size_t)r * pitch + se] < -eps) ? 2 : 0;
                if (lane == 0) {
                    pub[1] = r;
                    pub[2] = act;
                }
            }
#else
            if (wave == 0) {
                auto ratio = [&](int i) -> double {
                    const double a = T[(size_t)i * pitch + se], xb = T[(size_t)i * pitch + n];
                    const double u = ubound(basis[i]);
                    return (a > eps) ? xb / a : (a < -eps && u < INFINITY) ? (xb - u) / a : INFINITY;
                };
                int r;
                if (m <= 128) {
                    double rv[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int i = lane + 64 * k;
                        rv[k] = (i < m) ? ratio(i) : INFINITY;
                    }
                    r = wave_ratio_select<2>(rv, m, eps);
                } else if (m <= 256) {
                    double rv[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int i = lane + 64 * k;
                        rv[k] = (i < m) ? ratio(i) : INFINITY;
                    }
                    r = wave_ratio_select<4>(rv, m, eps);
                } else {
                    double theta;
                    auto getr = [&](int i, double& v, int& k, bool& ok) {
                        v = ratio(i);
                        k = i;
                        ok = true;
                    };
                    r = wave_scan_keyed<false>(m, eps, theta, getr);
                }
                const double ue = ubound(slotvar[se]);
                int act;
                if (r < 0) act = (ue < INFINITY) ? 1 : -1;
                else if (ue <= ratio(r)) act = 1;   // (theta: the selected row's value, the same division)
                else act = (T[(size_t)r * pitch + se] < -eps) ? 2 : 0;
#ifdef LP_BOUNDED_DEVEX
                if (act == 0 || act == 2) {
                    // weights from the old row r, the old pivot element and the entering slot's old weight.  Read ahead
                    // of the complement: that changes the sign of the row and of u_r alike, so t, t * t and u_r * u_r
                    // have the bits they have after it.  Slot se will hold the leaving variable.
                    const double ur = T[(size_t)r * pitch + se], we = wts[se];
                    for (int s = lane; s < n; s += 64)
                        if (s != se) {
                            const double t = T[(size_t)r * pitch + s] / ur;
                            wts[s] = fmax(wts[s], (t * t) * we);
                        }
                    if (lane == 0) wts[se] = fmax(we / (ur * ur), 1.0);
                }
#endif
                if (lane == 0) {
                    pub[1] = r;
                    pub[2] = act;
                }
            }
#endif
            __syncthreads();
            const int act = pub[2];
            if (act < 0) return LP_UNBOUNDED;
            if (act == 1) {
                // bound flip: the entering variable crosses to its other bound; xB (cost row's rhs included) moves by
                // U_e times its column, then the column is negated
                const int e = slotvar[se];
                const double ue = U[e];
                for (int i = tid; i <= m; i += NT) {
                    double* te = T + (size_t)i * pitch + se;
                    double* xb = T + (size_t)i * pitch + n;
                    *xb = fma(-ue, *te, *xb);
                    *te = -*te;
                }
                if (tid == 0) up[e] ^= 1;
                ++flips;
                __syncthreads();
            } else {
                const int r = pub[1];
                if (act == 2) {
                    // the leaving variable reaches its upper bound: hold its complement (row r's slots negated,
                    // xB_r = U_r - xB_r), which then leaves at 0
                    const int k = basis[r];
                    for (int j = tid; j < n; j += NT) T[(size_t)r * pitch + j] = -T[(size_t)r * pitch + j];
                    if (tid == 0) {
                        T[(size_t)r * pitch + n] = U[k] - T[(size_t)r * pitch + n];
                        up[k] ^= 1;
                    }
                    __syncthreads();
                }
                pivot(r, se);
                ++pivots;
            }
            if (++count >= d.max_iter) return LP_ITER_LIMIT;
        }
    };
