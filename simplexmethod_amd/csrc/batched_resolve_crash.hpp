// batched_resolve_crash.hpp — the basis install of the one-LP-per-workgroup kernels that start from a given basis
// (batched_resolve.hip, basis_parametric.hip), included INSIDE each kernel after batched_lds_loop.hpp and after it
// has defined `identity` (the slack-identity test), `status` (LP_OPTIMAL) and N (the basis by position).  Not a
// standalone header.  It is resolve_ref.c's crash: skipped for the slack identity with zero costs, else m forced
// pivots on the first-max |T[i][N(t)]| over the rows still held by an artificial, the singular verdict, then the
// rows permuted in place into basis-position order (every one of the W stored columns moves with its row).
    if (identity) {   // the basic columns are the artificials' own: bar their slots
        for (int t = tid; t < m; t += NT) {
            slotvar[N[t]] = n + t;
            basis[t] = N[t];
        }
        __syncthreads();
    } else {
        // ---- crash: m forced pivots; wave 0 keeps the smallest and largest pivot magnitude (wave-uniform)
        double minp = INFINITY, maxp = 0.0;
        for (int t = 0; t < m; ++t) {
            const int q = N[t];
            if (wave == 0) {
                int p = -1;
                // (a variable that is basic already — a repeated column — has only zeros in the unused rows)
                if (slotvar[q] == q) {
                    double big = -1.0;
                    int pi = INT_MAX;
                    for (int i = lane; i < m; i += 64) {
                        if (basis[i] < n) continue;   // row used by an earlier pivot
                        const double a = fabs(T[(size_t)i * pitch + q]);
                        if (a > big) {   // i ascending per lane: strict > keeps the first maximum
                            big = a;
                            pi = i;
                        }
                    }
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const double ob = __shfl_xor(big, off, 64);
                        const int op = __shfl_xor(pi, off, 64);
                        if (ob > big || (ob == big && op < pi)) {
                            big = ob;
                            pi = op;
                        }
                    }
                    if (big > 0.0) {
                        p = pi;
                        if (big < minp) minp = big;
                        if (big > maxp) maxp = big;
                    }
                }
                if (lane == 0) pub[0] = p;
            }
            __syncthreads();
            const int p = pub[0];
            if (p < 0) {
                status = LP_SINGULAR;
                break;
            }
            pivot(p, q);
        }
        if (status == LP_OPTIMAL) {
            if (tid == 0) pub[2] = minp <= DBL_EPSILON * (double)m * maxp;
            __syncthreads();
            if (pub[2]) status = LP_SINGULAR;
        }
        if (status == LP_OPTIMAL) {
            // ---- rows into basis-position order: new row t = old row rowpos[t], one cycle at a time
            int* rowpos = reinterpret_cast<int*>(lcol);
            for (int t = tid; t < m; t += NT) {
                const int q = N[t];
                int p = 0;
                for (int i = 0; i < m; ++i)
                    if (basis[i] == q) p = i;
                rowpos[t] = p;
            }
            __syncthreads();
            for (int t0 = 0; t0 < m; ++t0) {
                if (rowpos[t0] == t0) continue;
                for (int j = tid; j < W; j += NT) prow[j] = T[(size_t)t0 * pitch + j];
                __syncthreads();
                int t = t0;
                for (;;) {
                    const int src = rowpos[t];
                    if (src == t0) break;
                    for (int j = tid; j < W; j += NT) T[(size_t)t * pitch + j] = T[(size_t)src * pitch + j];
                    __syncthreads();
                    t = src;
                }
                for (int j = tid; j < W; j += NT) T[(size_t)t * pitch + j] = prow[j];
                __syncthreads();
                if (tid == 0)   // the cycle is in place
                    for (int u = t0; rowpos[u] != u;) {
                        const int next = rowpos[u];
                        rowpos[u] = u;
                        u = next;
                    }
                __syncthreads();
            }
            for (int t = tid; t < m; t += NT) basis[t] = N[t];
            __syncthreads();
        }
    }
