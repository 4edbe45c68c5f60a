// batched_bounded_dual_loop.hpp — the bounded-variable dual simplex loop of batched_bounded_resolve.hip
// (tests/ref/bounded_resolve_ref.c step 6), included INSIDE the kernel after batched_lds_loop.hpp (it calls pivot) and
// after the kernel has defined the LDS carve (T, pitch, U, up, slotvar, basis, pub), m, n, eps, maximize, tid, wave,
// lane and d.max_iter.  Every basic variable is a structural one here (the crash has run).  Not a standalone header.
//
// Wave 0 selects.  The leaving position is the EPS-hysteresis chain (min, position order) over the violated
// positions: v = xB below 0, else U - xB for a finite U below 0.  A position violated above is complemented before
// it leaves (row r's n slots negated, xB_r = U_r - xB_r, the flag toggled), so the entering chain reads row r with that
// sign already applied: q = d / a (max) or -d / a (min) over the slots holding a variable < n with a < -eps, in
// variable order.  pub[0] entering slot, pub[1] leaving position, pub[2] complement first: every wave takes the same
// branch.
//
// Under the macro LP_BOUNDED_DUAL_DEVEX (the _ddevex kernels of batched_bounded_resolve.hip, with the carve's dwts, one
// double per basis position; tests/ref/bounded_resolve_dual_rules_ref.c states the rule) the loop sets the weights to
// 1.0 when it starts, and the leaving position is the violated one of largest (v * v) / w, exact ties to the smallest
// position, without eps.  Between the complement and the pivot every thread updates the weights from column se:
// w_i = cand if cand = (g * g) * w_r > w_i with g = T[i][se] / a, a = T[r][se] as the complement left it, then
// w_r = max(w_r / (a * a), 1.0) by the thread that owns r.  a and the old w_r are read ahead of a barrier of their
// own, so no thread reads w_r after its owner has rewritten it.  Without the macro the code is what it was.
//
// Under the macro LP_BOUNDED_DUAL_LONG_STEP (the _long kernels of batched_bounded_resolve.hip;
// tests/ref/bounded_resolve_long_step_ref.c states the rule) the entering step is the bound-flipping ratio test.  Wave 0
// publishes with its candidate whether it is to be flipped (bit 1 of pub[2]): U_e finite and
// fma(-U_e, a, xB_r) < -eps on the complemented row r, so that row r stays violated with e at its other bound.  Every
// thread then does batched_bounded_loop.hpp's flip on column se and the xB column, rows 0 .. m; one barrier; wave 0
// rescans row r, which holds its complement by then, with the same keyed scan (the flipped slot has a > eps now and
// nothing else of row r or of the cost row changed, so no mask is needed) and publishes again.  The loop takes
// `flips` as a second counter; max_iter bounds the pivots alone.  Without the macro the code is what it was.
#ifdef LP_BOUNDED_DUAL_LONG_STEP
    auto bounded_dual = [&](int& iters, int& flips) -> int {
#else
    auto bounded_dual = [&](int& iters) -> int {
#endif
        if (d.max_iter <= 0) return LP_ITER_LIMIT;
#ifdef LP_BOUNDED_DUAL_DEVEX
        for (int t = tid; t < m; t += NT) dwts[t] = 1.0;
        __syncthreads();
#endif
        for (;;) {
            if (wave == 0) {
                double best;
#ifdef LP_BOUNDED_DUAL_DEVEX
                const int r0 = wave_argmax_keyed(m, [&](int t, double& v, int& k, bool& ok) {
                    const double xb = T[(size_t)t * pitch + n], u = U[basis[t]];
                    double viol = xb;
                    ok = true;
                    if (!(xb < -eps)) {
                        viol = u - xb;
                        ok = u < INFINITY && viol < -eps;
                    }
                    v = (viol * viol) / dwts[t];
                    k = t;
                });
#else
                const int r0 = wave_scan_keyed<false>(m, eps, best, [&](int t, double& v, int& k, bool& ok) {
                    const double xb = T[(size_t)t * pitch + n], u = U[basis[t]];
                    k = t;
                    if (xb < -eps) {
                        v = xb;
                        ok = true;
                    } else {
                        v = u - xb;
                        ok = u < INFINITY && v < -eps;
                    }
                });
#endif
                int se0 = -1, comp = 0;
                if (r0 >= 0) {
                    const double* rrow = T + (size_t)r0 * pitch;
                    const double* drow = T + (size_t)m * pitch;
                    comp = !(rrow[n] < -eps);
                    se0 = wave_scan_keyed<false>(n, eps, best, [&](int s, double& v, int& k, bool& ok) {
                        const double a = comp ? -rrow[s] : rrow[s];
                        k = slotvar[s];
                        ok = k < n && a < -eps;
                        v = maximize ? drow[s] / a : -drow[s] / a;
                    });
                }
#ifdef LP_BOUNDED_DUAL_LONG_STEP
                if (se0 >= 0) {   // flip se0 first? (row r0 as the complement below will leave it)
                    const double* rrow = T + (size_t)r0 * pitch;
                    const double a = comp ? -rrow[se0] : rrow[se0];
                    const double xbr = comp ? U[basis[r0]] - rrow[n] : rrow[n];
                    const double ue = U[slotvar[se0]];
                    if (ue < INFINITY && fma(-ue, a, xbr) < -eps) comp |= 2;
                }
#endif
                if (lane == 0) {
                    pub[0] = se0;
                    pub[1] = r0;
                    pub[2] = comp;
                }
            }
            __syncthreads();
#ifdef LP_BOUNDED_DUAL_LONG_STEP
            int se = pub[0];
            const int r = pub[1];
            int flip = pub[2] & 2;
            if (r < 0) return LP_OPTIMAL;
            if (pub[2] & 1) {
#else
            const int se = pub[0], r = pub[1];
            if (r < 0) return LP_OPTIMAL;
            if (pub[2]) {
#endif
                const int k = basis[r];
                for (int j = tid; j < n; j += NT) T[(size_t)r * pitch + j] = -T[(size_t)r * pitch + j];
                if (tid == 0) {
                    T[(size_t)r * pitch + n] = U[k] - T[(size_t)r * pitch + n];
                    up[k] ^= 1;
                }
                __syncthreads();
            }
            if (se < 0) return LP_INFEASIBLE;
#ifdef LP_BOUNDED_DUAL_LONG_STEP
            while (flip) {
                // bound flip (batched_bounded_loop.hpp's): row r stays violated with the candidate at its other bound
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
                if (wave == 0) {
                    double best;
                    const double* rrow = T + (size_t)r * pitch;
                    const double* drow = T + (size_t)m * pitch;
                    const int se0 = wave_scan_keyed<false>(n, eps, best, [&](int s, double& v, int& k, bool& ok) {
                        const double a = rrow[s];
                        k = slotvar[s];
                        ok = k < n && a < -eps;
                        v = maximize ? drow[s] / a : -drow[s] / a;
                    });
                    int again = 0;
                    if (se0 >= 0) {
                        const double u2 = U[slotvar[se0]];
                        again = (u2 < INFINITY && fma(-u2, rrow[se0], rrow[n]) < -eps) ? 2 : 0;
                    }
                    if (lane == 0) {
                        pub[0] = se0;
                        pub[2] = again;
                    }
                }
                __syncthreads();
                se = pub[0];
                flip = pub[2];
                if (se < 0) return LP_INFEASIBLE;
            }
#endif
#ifdef LP_BOUNDED_DUAL_DEVEX
            {
                const double a = T[(size_t)r * pitch + se], wr = dwts[r];
                __syncthreads();
                for (int i = tid; i < m; i += NT) {
                    if (i == r) {
                        dwts[i] = fmax(wr / (a * a), 1.0);
                    } else {
                        const double g = T[(size_t)i * pitch + se] / a;
                        const double cand = (g * g) * wr;
                        if (cand > dwts[i]) dwts[i] = cand;
                    }
                }
            }
#endif
            pivot(r, se);
            ++iters;
            if (iters >= d.max_iter) return LP_ITER_LIMIT;
        }
    };
