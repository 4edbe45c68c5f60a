// basis_certificate.hip — Farkas and unbounded-ray certificates at a given basis, exactly as
// tests/ref/certificate_ref.c states them:
//   - a basis index n+i is the artificial of row i, column s_i e_i (s_i = -1 when b[i] < -eps, else +1);
//   - Binv and xB by ranging's crash on [B | I | b] (basis_crash.hpp, kept in place in m x (m+1));
//   - alpha[t][j] = sum_i Binv[t][i] A[i][j], one fma chain per entry in row order, built only where the case
//     needs it;
//   - phase-I case (an artificial is basic): f = -(sum of Binv's artificial rows), FARKAS when the artificials'
//     values sum > eps and f^T A_j >= -eps for every original j;
//   - dual-simplex case (no artificial, some xB[t] < -eps): the first such t whose alpha row is >= -eps on the
//     non-basic columns, f = Binv[t][:];
//   - ray case (otherwise): d_j = c_j - sum_t c_B[t] alpha[t][j] in position order, the first non-basic j that
//     improves by more than eps with alpha[t][j] <= eps for every t.
//
// k_batched_certificate: one LP per workgroup, state in LDS.  The case is chosen once per workgroup from the
// basis and xB (block-uniform).  The alpha chains run one column per thread of the first kCW threads, kR weight
// rows at a time, against A tiles staged through LDS.
//
// Shapes beyond lp_basis_certificate_fits: k_certificate_gather builds [B | I | b; 0] with the artificial columns
// explicit, the single-LP launch pair (lp_simplex_crash) pivots it, k_binv_times_a (basis_ranging.hip) forms
// B^-1 A, then k_cert_prepare, k_cert_columns and k_cert_finish choose the case and reduce.
#include <cfloat>

#include "basis_col_chains.hpp"
#include "basis_crash.hpp"
#include "batched_problem.hpp"
#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

constexpr int kR = 8;      // weight rows per alpha pass

__host__ __device__ inline int certificate_threads(int m) { return m <= 64 ? 256 : 512; }
__host__ __device__ inline int certificate_pitch(int m) { return (m + 1) | 1; }
// doubles of the region that holds lcol + prow during the crash, then the A tiles
__host__ __device__ inline size_t certificate_scratch(int m) {
    const size_t tile = (size_t)kCW * (kTR + 1), eta = 2 * (size_t)m + 1;
    return tile > eta ? tile : eta;
}

template <int NT, bool MX>
__global__ __launch_bounds__(NT) void k_batched_certificate(BasisCertificateDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int m = d.m, n = d.n, pitch = certificate_pitch(m);
    const int tid = threadIdx.x;
    const int lp = blockIdx.x;
    const double eps = d.eps;
    // ---- LDS carve
    int* pub = reinterpret_cast<int*>(smem);        // [0] pivot row, [1] singular verdict, [2] block_any, [3] pick
    double* T = smem + 2;                           // m x pitch
    double* U = T + (size_t)m * pitch;              // lcol + prow | the A tiles
    double* fv = U + certificate_scratch(m);        // m: f, or the ray's alpha column
    int* rowpos = reinterpret_cast<int*>(fv + m);   // m
    int* used = rowpos + m;                         // m: the crash's flags, then a position list
    int* zneg = used + m;                           // m
    int* slot = zneg + m;                           // m: slot[i] holds identity column m+i
    int* pos = slot + m;                            // n: position of a basic original column, -1 otherwise
    int* okr = pos + n;                             // kR
    double* lcol = U;
    double* prow = U + m;

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const int* N = d.basis + (size_t)lp * m;
    double* farkas = d.farkas + (size_t)lp * m;
    double* ray = d.ray + (size_t)lp * n;
    constexpr int ANY_WORD = 2;   // block_any's word of pub
#include "batched_block_any.hpp"
    auto binv = [&](int t, int i) { return T[(size_t)rowpos[t] * pitch + slot[i]]; };
    auto xb = [&](int t) { return T[(size_t)rowpos[t] * pitch + m]; };

    const int run = d.run_status ? d.run_status[lp] : LP_OPTIMAL;
    int status = LP_OPTIMAL;   // the certificate's own
    int kind = LP_CERT_NONE, index = -1;
    const bool eligible = !d.run_status || run == LP_INFEASIBLE || run == LP_UNBOUNDED;
    if (eligible) {
        int bad = 0, rep = 0;
        for (int t = tid; t < m; t += NT) {
            if (N[t] < 0 || N[t] >= n + m) bad = 1;
            for (int u = 0; u < t; ++u)
                if (N[u] == N[t]) rep = 1;
        }
        if (block_any(bad)) status = LP_BAD_ARG;
        else if (block_any(rep)) status = LP_SINGULAR;
    }
    if (eligible && status == LP_OPTIMAL) {
        // ---- [B | I | b] in place: T[i][t] = column N[t] (A's, or s_i e_i for an artificial), T[i][m] = b[i]
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m, k = N[t];
            T[(size_t)i * pitch + t] = k < n ? A[(size_t)k * m + i] : (k - n == i ? (b[i] < -eps ? -1.0 : 1.0) : 0.0);
        }
        for (int i = tid; i < m; i += NT) {
            T[(size_t)i * pitch + m] = b[i];
            used[i] = 0;
            zneg[i] = 0;
        }
        __syncthreads();
        status = ranging_crash<NT, true>(T, m, pitch, lcol, prow, used, rowpos, zneg, pub);
    }
    const bool on = eligible && status == LP_OPTIMAL;
    if (on) {
        for (int s = tid; s < m; s += NT) slot[rowpos[s]] = s;
        for (int j = tid; j < n; j += NT) pos[j] = -1;
        for (int i = tid; i < m; i += NT) used[i] = -1;   // now: the position of artificial n+i
        __syncthreads();
        int art = 0, neg = 0;
        for (int t = tid; t < m; t += NT) {
            if (N[t] < n) {
                pos[N[t]] = t;
            } else {
                used[N[t] - n] = t;
                art = 1;
            }
            if (xb(t) < -eps) neg = 1;
        }
        const bool any_art = block_any(art);
        const bool any_neg = block_any(neg);
        double* tile = U;
        if (any_art) {
            // ---- phase-I case: f, the artificials' sum, then every f^T A_j
            for (int i = tid; i < m; i += NT) {
                double u = 0.0;
                for (int t = 0; t < m; ++t)
                    if (N[t] >= n) u = u + binv(t, i);
                fv[i] = -u;
            }
            if (tid == 0) {
                double sum = 0.0;
                for (int i = 0; i < m; ++i)
                    if (used[i] >= 0) sum = sum + xb(used[i]);
                pub[3] = sum > eps;
            }
            __syncthreads();
            bool ok = pub[3] != 0;
            const int rp[1] = {0};
            for (int j0 = 0; j0 < n && ok; j0 += kCW) {
                double g[1];
                col_chains<NT, 1>(A, m, n, j0, tile, fv, rp, nullptr, g);
                ok = !block_any(tid < kCW && j0 + tid < n && !(g[0] >= -eps));
            }
            if (ok) kind = LP_CERT_FARKAS;
        } else if (any_neg) {
            // ---- dual-simplex case: the candidate positions in order, kR alpha rows per pass
            if (tid == 0) {
                int q = 0;
                for (int t = 0; t < m; ++t)
                    if (xb(t) < -eps) used[q++] = t;
                pub[3] = q;
            }
            __syncthreads();
            const int nc = pub[3];
            for (int c0 = 0; c0 < nc && kind == LP_CERT_NONE; c0 += kR) {
                int rp[kR];
#pragma unroll
                for (int r = 0; r < kR; ++r) rp[r] = rowpos[used[c0 + r < nc ? c0 + r : c0]] * pitch;
                if (tid < kR) okr[tid] = 1;
                for (int j0 = 0; j0 < n; j0 += kCW) {
                    double acc[kR];
                    col_chains<NT, kR>(A, m, n, j0, tile, T, rp, slot, acc);
                    const int j = j0 + tid;
                    if (tid < kCW && j < n && pos[j] < 0)
#pragma unroll
                        for (int r = 0; r < kR; ++r)
                            if (!(acc[r] >= -eps)) okr[r] = 0;
                }
                __syncthreads();
                for (int r = 0; r < kR && c0 + r < nc; ++r)
                    if (okr[r]) {
                        kind = LP_CERT_FARKAS;
                        index = used[c0 + r];
                        break;
                    }
                __syncthreads();   // okr: every reader is done before the next pass resets it
            }
            if (kind == LP_CERT_FARKAS)
                for (int i = tid; i < m; i += NT) fv[i] = binv(index, i);
        } else {
            // ---- ray case: per column d_j and the alpha <= eps test over every position, kR positions per pass
            if (tid == 0) pub[3] = INT_MAX;
            double dwin = 0.0;
            for (int j0 = 0; j0 < n; j0 += kCW) {
                const int j = j0 + tid;
                const bool col = tid < kCW && j < n && pos[j] < 0;
                double dj = col ? c[j] : 0.0;
                bool ok = true;
                for (int t0 = 0; t0 < m; t0 += kR) {
                    int rp[kR];
#pragma unroll
                    for (int r = 0; r < kR; ++r) rp[r] = rowpos[t0 + r < m ? t0 + r : t0] * pitch;
                    double acc[kR];
                    col_chains<NT, kR>(A, m, n, j0, tile, T, rp, slot, acc);
#pragma unroll
                    for (int r = 0; r < kR; ++r)
                        if (t0 + r < m) {
                            dj = fma(-c[N[t0 + r]], acc[r], dj);
                            if (!(acc[r] <= eps)) ok = false;
                        }
                }
                if (col && ok && (MX ? dj > eps : dj < -eps)) atomicMin(&pub[3], j);
                __syncthreads();
                const int w = pub[3];
                if (w != INT_MAX) {
                    if (j == w) fv[0] = dj;   // (fv is free until the winner's column below)
                    __syncthreads();
                    dwin = fv[0];
                    __syncthreads();
                    kind = LP_CERT_RAY;
                    index = w;
                    break;
                }
            }
            if (kind == LP_CERT_RAY) {
                // the winner's alpha column, one chain per position, then r
                for (int t = tid; t < m; t += NT) {
                    double s = 0.0;
                    for (int i = 0; i < m; ++i) s = fma(binv(t, i), A[(size_t)index * m + i], s);
                    fv[t] = s;
                }
                __syncthreads();
                for (int k = tid; k < n; k += NT) ray[k] = k == index ? 1.0 : pos[k] >= 0 ? -fv[pos[k]] : 0.0;
                if (tid == 0) d.value[lp] = dwin;
            }
        }
    }
    // ---- outputs (f was filled by every wave: thread 0 reads all of it for b^T f)
    __syncthreads();
    if (kind == LP_CERT_FARKAS) {
        for (int i = tid; i < m; i += NT) farkas[i] = fv[i];
        if (tid == 0) {
            double v = 0.0;
            for (int i = 0; i < m; ++i) v = fma(b[i], fv[i], v);
            d.value[lp] = v;
        }
    } else {
        for (int i = tid; i < m; i += NT) farkas[i] = NAN;
    }
    if (kind != LP_CERT_RAY)
        for (int k = tid; k < n; k += NT) ray[k] = NAN;
    if (tid == 0) {
        if (kind == LP_CERT_NONE) d.value[lp] = NAN;
        d.kind[lp] = kind;
        d.index[lp] = index;
        d.status[lp] = !eligible ? run : status != LP_OPTIMAL ? status : run;
    }
}

template <int NT, bool MX>
int batched_certificate_launch(lp_context* ctx, const BasisCertificateDev& d) {
    return lp_launch_per_lp(ctx, k_batched_certificate<NT, MX>, NT, lp_basis_certificate_lds_bytes(d.m, d.n), d);
}

// ---- the single-LP path beyond lp_basis_certificate_fits

// T (m+1 rows, pitch ld) = [B | I | b; 0] with artificial n+i as s_i e_i; the crash bookkeeping's basis = 0..m-1
__global__ __launch_bounds__(256) void k_certificate_gather(SimplexDev s, const double* A, int n, const double* b,
                                                            const int* basis, double eps) {
    const int i = blockIdx.x;   // tableau row, 0..m
    const int m = s.m;
    double* row = s.T + (size_t)i * s.ld;
    if (i == m) {
        for (int j = threadIdx.x; j < s.ld; j += blockDim.x) row[j] = 0.0;
        return;
    }
    const double si = b[i] < -eps ? -1.0 : 1.0;
    for (int j = threadIdx.x; j < s.ld; j += blockDim.x) {
        double v = 0.0;
        if (j < m) v = basis[j] < n ? A[(size_t)basis[j] * m + i] : (basis[j] - n == i ? si : 0.0);
        else if (j < 2 * m) v = j - m == i ? 1.0 : 0.0;
        else if (j == 2 * m) v = b[i];
        row[j] = v;
    }
    if (threadIdx.x == 0) s.basis[i] = i;
}

// Scratch of the single-LP reductions (device).
struct CertScratch {
    int cas;      // 0 phase I, 1 dual simplex, 2 ray
    int ok;       // phase I: the artificials' sum > eps and no g_j < -eps so far
    int best;     // ray: the first qualifying column (atomicMin), INT_MAX for none
    int pad;
};

// One block: the case, pos (n + m: position of a basic index, -1 otherwise), f and the sum test of phase I
__global__ __launch_bounds__(256) void k_cert_prepare(SimplexDev s, int n, const int* basis, double eps, int* pos,
                                                      double* f, CertScratch* cs) {
    __shared__ int flags[2];
    const int m = s.m, ld = s.ld, tid = threadIdx.x;
    if (tid == 0) flags[0] = flags[1] = 0;
    for (int k = tid; k < n + m; k += 256) pos[k] = -1;
    __syncthreads();
    for (int t = tid; t < m; t += 256) {
        pos[basis[t]] = t;
        if (basis[t] >= n) flags[0] = 1;
        if (s.T[(size_t)t * ld + 2 * m] < -eps) flags[1] = 1;
    }
    __syncthreads();
    const int cas = flags[0] ? 0 : flags[1] ? 1 : 2;
    if (cas == 0)
        for (int i = tid; i < m; i += 256) {
            double u = 0.0;
            for (int t = 0; t < m; ++t)
                if (basis[t] >= n) u = u + s.T[(size_t)t * ld + m + i];
            f[i] = -u;
        }
    if (tid == 0) {
        double sum = 0.0;
        if (cas == 0)
            for (int i = 0; i < m; ++i)
                if (pos[n + i] >= 0) sum = sum + s.T[(size_t)pos[n + i] * ld + 2 * m];
        cs->cas = cas;
        cs->ok = cas == 0 && sum > eps;
        cs->best = INT_MAX;
    }
}

// One thread per original column j: phase I g_j; dual simplex the alpha test of every candidate row (bad[t]);
// ray d_j (dd[j]) and its qualification
template <bool MX>
__global__ __launch_bounds__(256) void k_cert_columns(SimplexDev s, const double* A, int n, const double* c,
                                                      const int* basis, const double* alpha, const double* f,
                                                      const int* pos, double eps, int* bad, double* dd,
                                                      CertScratch* cs) {
    const int m = s.m, ld = s.ld;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int cas = cs->cas;
    if (cas == 0) {
        if (!cs->ok) return;
        double g = 0.0;
        for (int i = 0; i < m; ++i) g = fma(f[i], A[(size_t)j * m + i], g);
        if (!(g >= -eps)) cs->ok = 0;
        return;
    }
    if (pos[j] >= 0) return;
    if (cas == 1) {
        for (int t = 0; t < m; ++t)
            if (s.T[(size_t)t * ld + 2 * m] < -eps && !(alpha[(size_t)t * n + j] >= -eps)) bad[t] = 1;
        return;
    }
    double dj = c[j];
    bool ok = true;
    for (int t = 0; t < m; ++t) {
        const double a = alpha[(size_t)t * n + j];
        dj = fma(-c[basis[t]], a, dj);
        if (!(a <= eps)) ok = false;
    }
    dd[j] = dj;
    if (ok && (MX ? dj > eps : dj < -eps)) atomicMin(&cs->best, j);
}

// One block: the outputs
__global__ __launch_bounds__(256) void k_cert_finish(SimplexDev s, int n, const double* b, const double* alpha,
                                                     const double* f, const int* pos, double eps, const int* bad,
                                                     const double* dd, const CertScratch* cs, int* kind_out,
                                                     double* farkas, double* ray, double* value_out,
                                                     int* index_out) {
    __shared__ int pick[2];   // kind, index
    const int m = s.m, ld = s.ld, tid = threadIdx.x;
    const int cas = cs->cas;
    if (tid == 0) {
        int kind = LP_CERT_NONE, index = -1;
        if (cas == 0) {
            if (cs->ok) kind = LP_CERT_FARKAS;
        } else if (cas == 1) {
            for (int t = 0; t < m; ++t)
                if (s.T[(size_t)t * ld + 2 * m] < -eps && !bad[t]) {
                    kind = LP_CERT_FARKAS;
                    index = t;
                    break;
                }
        } else if (cs->best != INT_MAX) {
            kind = LP_CERT_RAY;
            index = cs->best;
        }
        pick[0] = kind;
        pick[1] = index;
    }
    __syncthreads();
    const int kind = pick[0], index = pick[1];
    // f: phase I's, or row `index` of B^-1
    auto fi = [&](int i) { return cas == 0 ? f[i] : s.T[(size_t)index * ld + m + i]; };
    for (int i = tid; i < m; i += 256) farkas[i] = kind == LP_CERT_FARKAS ? fi(i) : NAN;
    for (int k = tid; k < n; k += 256)
        ray[k] = kind != LP_CERT_RAY ? NAN
                 : k == index        ? 1.0
                 : pos[k] >= 0       ? -alpha[(size_t)pos[k] * n + index]
                                     : 0.0;
    if (tid == 0) {
        double v = NAN;
        if (kind == LP_CERT_FARKAS) {
            v = 0.0;
            for (int i = 0; i < m; ++i) v = fma(b[i], fi(i), v);
        } else if (kind == LP_CERT_RAY) {
            v = dd[index];
        }
        *kind_out = kind;
        *value_out = v;
        *index_out = index;
    }
}

}  // namespace

size_t lp_basis_certificate_lds_bytes(int m, int n) {
    // pub (2 doubles), T, the scratch region, fv; rowpos + used + zneg + slot, pos, okr
    return sizeof(double) * (2 + (size_t)m * certificate_pitch(m) + certificate_scratch(m) + (size_t)m) +
           sizeof(int) * (4 * (size_t)m + n + kR);
}

int lp_basis_certificate_launch(lp_context* ctx, const BasisCertificateDev& d) {
    if (!lp_basis_certificate_fits(d.m, d.n))
        LP_FAIL(ctx, LP_BAD_ARG, "basis certificate: the shape does not fit one CU's LDS");
    if (d.batch <= 0) return LP_OPTIMAL;
    if (certificate_threads(d.m) == 256)
        return d.maximize ? batched_certificate_launch<256, true>(ctx, d)
                          : batched_certificate_launch<256, false>(ctx, d);
    return d.maximize ? batched_certificate_launch<512, true>(ctx, d) : batched_certificate_launch<512, false>(ctx, d);
}

// One LP of any size on the device: A, b, c, basis already there (range and repeats checked by the caller).
int lp_basis_certificate_device(lp_context* ctx, const double* dA, int m, int n, const double* db, const double* dc,
                                const int* dbasis, int maximize, double eps, int* dkind, double* dfarkas,
                                double* dray, double* dvalue, int* dindex) {
    hipStream_t s = ctx->stream;
    const int ld = (int)lp_ceil_div<size_t>(2 * (size_t)m + 1, 8) * 8;
    lp_simplex_problem q;
    q.ctx = ctx;
    q.tableau_bytes = sizeof(double) * (size_t)(m + 1) * ld;
    SimplexDev& sd = q.dev;
    sd.m = m;
    sd.n = 2 * m;   // the right-hand-side column of [B | I | b]
    sd.ld = ld;
    // one allocation: T, the pristine copy the crash permutes through, lcol, prow, state, basis, rowpos, rowused;
    // alpha, f, d, pos, bad and the scratch record
    double *alpha, *f, *dd;
    int *pos, *bad;
    CertScratch* cs;
    auto pieces = [&](lp_carver& cv) {
        sd.T = cv.take<double>(q.tableau_bytes);
        q.dT0 = cv.take<double>(q.tableau_bytes);
        sd.lcol = cv.take<double>(sizeof(double) * ((size_t)m + 1));
        sd.prow = cv.take<double>(sizeof(double) * (size_t)ld);
        sd.state = cv.take<SimplexState>(sizeof(SimplexState));
        sd.basis = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowpos = cv.take<int>(sizeof(int) * (size_t)m);
        sd.rowused = cv.take<unsigned char>((size_t)m);
        alpha = cv.take<double>(sizeof(double) * (size_t)m * n);
        f = cv.take<double>(sizeof(double) * (size_t)m);
        dd = cv.take<double>(sizeof(double) * (size_t)n);
        pos = cv.take<int>(sizeof(int) * ((size_t)n + m));
        bad = cv.take<int>(sizeof(int) * (size_t)m);
        cs = cv.take<CertScratch>(sizeof(CertScratch));
    };
    char* arena = nullptr;
    LP_HIP(ctx, lp_carve_malloc(&arena, pieces));
    int rc = LP_OPTIMAL;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int) * (size_t)m, s);
    if (e != hipSuccess) rc = -(int)e;
    if (rc == LP_OPTIMAL) {
        hipLaunchKernelGGL(k_certificate_gather, m + 1, 256, 0, s, sd, dA, n, db, dbasis, eps);
        rc = lp_simplex_crash(&q);   // m launch pairs, the verdict, rows into position order; one host sync
    }
    if (rc == LP_OPTIMAL) {
        lp_binv_times_a_launch(ctx, sd, dA, n, alpha);
        hipLaunchKernelGGL(k_cert_prepare, 1, 256, 0, s, sd, n, dbasis, eps, pos, f, cs);
        if (maximize)
            hipLaunchKernelGGL(k_cert_columns<true>, lp_ceil_div(n, 256), 256, 0, s, sd, dA, n, dc, dbasis, alpha, f,
                               pos, eps, bad, dd, cs);
        else
            hipLaunchKernelGGL(k_cert_columns<false>, lp_ceil_div(n, 256), 256, 0, s, sd, dA, n, dc, dbasis, alpha,
                               f, pos, eps, bad, dd, cs);
        hipLaunchKernelGGL(k_cert_finish, 1, 256, 0, s, sd, n, db, alpha, f, pos, eps, bad, dd, cs, dkind, dfarkas,
                           dray, dvalue, dindex);
        e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->last_error = std::string("basis certificate: ") + hipGetErrorString(e);
            rc = -(int)e;
        }
    }
    (void)hipFree(arena);
    return rc;
}
