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
    auto bounded_dual = [&](int& iters) -> int {
        if (d.max_iter <= 0) return LP_ITER_LIMIT;
        for (;;) {
            if (wave == 0) {
                double best;
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
                if (lane == 0) {
                    pub[0] = se0;
                    pub[1] = r0;
                    pub[2] = comp;
                }
            }
            __syncthreads();
            const int se = pub[0], r = pub[1];
            if (r < 0) return LP_OPTIMAL;
            if (pub[2]) {
                const int k = basis[r];
                for (int j = tid; j < n; j += NT) T[(size_t)r * pitch + j] = -T[(size_t)r * pitch + j];
                if (tid == 0) {
                    T[(size_t)r * pitch + n] = U[k] - T[(size_t)r * pitch + n];
                    up[k] ^= 1;
                }
                __syncthreads();
            }
            if (se < 0) return LP_INFEASIBLE;
            pivot(r, se);
            ++iters;
            if (iters >= d.max_iter) return LP_ITER_LIMIT;
        }
    };
