// batched_dual_loop.hpp — the dual simplex loop of the one-LP-per-workgroup kernels whose tableau lives in LDS
// (batched_resolve.hip, batched_mip.hip), included INSIDE each kernel after batched_lds_loop.hpp (it calls pivot)
// and after it has defined `maximize`.  Not a standalone header; shared by inclusion for the reason
// batched_lds_loop.hpp gives.  The leaving position is the EPS-hysteresis chain (min) over xB_t < -eps in position
// order, the entering slot the same chain over q = d / T[r][s] (max) or -d / T[r][s] (min) of the slots holding a
// variable of index < n with T[r][s] < -eps, in variable-index order.
    auto dual = [&](int& iters) -> int {
        if (d.max_iter <= 0) return LP_ITER_LIMIT;
        for (;;) {
            if (wave == 0) {
                double best;
                const int r0 = wave_scan_keyed<false>(m, eps, best, [&](int t, double& v, int& k, bool& ok) {
                    v = T[(size_t)t * pitch + n];
                    k = t;
                    ok = v < -eps;
                });
                int se0 = -1;
                if (r0 >= 0) {
                    const double* rrow = T + (size_t)r0 * pitch;
                    const double* drow = T + (size_t)m * pitch;
                    se0 = wave_scan_keyed<false>(n, eps, best, [&](int s, double& v, int& k, bool& ok) {
                        const double a = rrow[s];
                        k = slotvar[s];
                        ok = k < n && a < -eps;
                        v = maximize ? drow[s] / a : -drow[s] / a;
                    });
                }
                if (lane == 0) {
                    pub[0] = se0;
                    pub[1] = r0;
                }
            }
            __syncthreads();
            const int se = pub[0], r = pub[1];
            if (r < 0) return LP_OPTIMAL;
            if (se < 0) return LP_INFEASIBLE;
            pivot(r, se);
            ++iters;
            if (iters >= d.max_iter) return LP_ITER_LIMIT;
        }
    };
