/*
 * bounded_certificate_ref.c — TEST INFRASTRUCTURE ONLY: Farkas and unbounded-ray certificates of a bounded-variable LP
 * (opt c.x, A x = b, lo <= x <= hi, lo finite, hi finite or +inf) at a given basis and given at-upper flags: the
 * lp_basis_bounded_certificate family.  Everything is stated in the caller's original variables on the arithmetic of
 * certificate_ref.c and ranging_ref.c:
 *
 *   0. checks: eps < 0 or NaN, lo_j NaN or infinite, hi_j NaN, at_upper[j] not 0 or 1, or 1 with hi_j = +inf, basis[t]
 *      outside [0, n+m) -> REF_BAD_ARG.  Then any hi_j < lo_j -> REF_INFEASIBLE (crossed bounds need no vector), then a
 *      repeated index -> REF_SINGULAR.  A basis index n+i is the artificial of row i;
 *   1. held values: a non-basic column sits at v_j = hi_j if at_upper[j], else lo_j; the flag of a basic column is not
 *      read.  b'_i: the chain acc = fma(-A[i][j], v_j, acc) from acc = b_i over the non-basic j ascending with
 *      v_j != 0.0 (bounded_sens_ref.c step 3).  b0_i: the chain acc = fma(-A[i][j], lo_j, acc) from acc = b_i over every
 *      j ascending with lo_j != 0.0 (bounded_ref.c step 2).  The artificial of row i is the column s_i e_i with
 *      s_i = -1.0 when b0_i < -eps, else +1.0: the bounded two-phase's row flip, decided before anything is
 *      complemented;
 *   2. Binv and xB: ref_ranging_crash (explicit form) on [A | diag(s)] and b' (a singular crash: REF_SINGULAR).
 *      alpha[t][j] = (Binv A)[t][j] is the chain s = fma(Binv[t][i], A[i][j], s) for i ascending from s = 0;
 *   3. the sign test of a weight vector g over the original columns: every non-basic j has g_j >= -eps if held at lo_j
 *      and g_j <= eps if held at hi_j.  Basic columns are not tested; a fixed column is tested by its flag;
 *   4. Phase-I case (some basis[t] >= n): u[i] = the sum s = s + Binv[t][i] from s = 0 over the artificial positions t
 *      ascending, f[i] = -u[i]; g_j the chain fma(f[i], A[i][j], g) for i ascending from 0.  FARKAS iff the
 *      artificials' xB, in artificial-index order, summed from 0 with plain adds exceed eps and g passes 3.  value =
 *      the chain v = fma(b'[i], f[i], v) for i ascending from 0; index -1;
 *   5. Dual-simplex case (no artificial, some position violated): with L_t, H_t the bounds of basis[t], position t is
 *      violated below when xB[t] < L_t - eps, above when H_t < +inf and xB[t] > H_t + eps.  Over t ascending the first
 *      violated t whose row passes 3. gives FARKAS with index t: below f = Binv[t][:], g = alpha[t][:]; above
 *      f = -Binv[t][:], g = -alpha[t][:].  value = the chain of 4., then below: value - L_t when L_t != 0.0; above:
 *      value + H_t.  So value is xB[t] - L_t or H_t - xB[t] up to rounding;
 *   6. Ray case (otherwise): d_j = the chain s = fma(-c[basis[t]], alpha[t][j], s) for t ascending from s = c[j].  A
 *      candidate is a non-basic, unflagged j with hi_j = +inf and d_j > eps (max) or d_j < -eps (min); it is accepted
 *      when every t has alpha[t][j] <= eps, and alpha[t][j] >= -eps or H_t = +inf.  The first accepted j: r[j] = 1,
 *      r[basis[t]] = -alpha[t][j], +0.0 elsewhere; RAY, value d_j, index j;
 *   7. otherwise NONE.  farkas is NaN unless the kind is FARKAS, ray NaN unless it is RAY; value NaN and index -1 for
 *      NONE and whenever the status is not REF_OPTIMAL.  Every comparison is written so that a NaN fails it.
 *
 * What a certificate proves, with g = A^T f.  FARKAS: f.b < min over the box of f^T A x = sum_j min(g_j lo_j, g_j hi_j),
 * so no x in the box satisfies A x = b (f.b' = f.b - sum g_j v_j over the held columns, the minimising point of the
 * non-basic columns by 3.; the basic columns carry g_j = 0, or in 5. the violated bound of basis[t]).  RAY: A r = 0,
 * r >= -eps, r_k <= eps wherever hi_k is finite, and c.r = d_j of the improving sign.
 *
 * With lo = 0, hi = +inf and no flag every output is ref_certificate's bit for bit (the skipped-zero chains leave
 * b' = b0 = b, and L_t - eps = -eps).  Built with -ffp-contract=off (simplexmethod_amd/build.py:
 * build_bounded_certificate_ref).  Only tests load it.
 */
#include "certificate_ref.c"

enum { REF_INFEASIBLE = 4 };

/* step 3 for one non-basic column */
static int bcert_sign_ok(double g, int flagged, double eps) { return flagged ? g <= eps : g >= -eps; }

int ref_bounded_certificate(const double* A, int m, int n, const double* b, const double* c, const double* lo,
                            const double* hi, const int* basis, const int* at_upper, int maximize, double eps,
                            int* kind_out, double* farkas_out, double* ray_out, double* value_out, int* index_out) {
    if (m <= 0 || n < m || !A || !b || !c || !lo || !hi || !basis || !at_upper) return REF_BAD_ARG;
    if (!kind_out || !farkas_out || !ray_out || !value_out || !index_out) return REF_BAD_ARG;
    fill_cert_nan(m, n, kind_out, farkas_out, ray_out, value_out, index_out);
    /* 0. */
    if (!(eps >= 0.0)) return REF_BAD_ARG;
    for (int j = 0; j < n; ++j) {
        if (!isfinite(lo[j]) || isnan(hi[j])) return REF_BAD_ARG;
        if (at_upper[j] != 0 && at_upper[j] != 1) return REF_BAD_ARG;
        if (at_upper[j] && hi[j] == INFINITY) return REF_BAD_ARG;
    }
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n + m) return REF_BAD_ARG;
    for (int j = 0; j < n; ++j)
        if (hi[j] < lo[j]) return REF_INFEASIBLE;
    for (int t = 0; t < m; ++t)
        for (int u = 0; u < t; ++u)
            if (basis[u] == basis[t]) return REF_SINGULAR;

    const int na = n + m;
    int* pos = (int*)xmalloc(sizeof(int) * (size_t)na); /* position of a basic index, -1 otherwise */
    double* v = (double*)xmalloc(sizeof(double) * (size_t)n);
    double* bp = (double*)xmalloc(sizeof(double) * (size_t)m);
    double* Aa = (double*)xmalloc(sizeof(double) * (size_t)m * na);
    double* binv = (double*)xmalloc(sizeof(double) * (size_t)m * m);
    double* xb = (double*)xmalloc(sizeof(double) * (size_t)m);
    double* f = (double*)xmalloc(sizeof(double) * (size_t)m);
    double* col = (double*)xmalloc(sizeof(double) * (size_t)m);
    for (int k = 0; k < na; ++k) pos[k] = -1;
    for (int t = 0; t < m; ++t) pos[basis[t]] = t;
    /* 1. */
    for (int j = 0; j < n; ++j) v[j] = pos[j] >= 0 ? 0.0 : at_upper[j] ? hi[j] : lo[j];
    memcpy(Aa, A, sizeof(double) * (size_t)m * n);
    memset(Aa + (size_t)m * n, 0, sizeof(double) * (size_t)m * m);
    for (int i = 0; i < m; ++i) {
        double acc = b[i], b0 = b[i];
        for (int j = 0; j < n; ++j) {
            if (pos[j] < 0 && v[j] != 0.0) acc = fma(-AT(A, m, i, j), v[j], acc);
            if (lo[j] != 0.0) b0 = fma(-AT(A, m, i, j), lo[j], b0);
        }
        bp[i] = acc;
        AT(Aa, m, i, n + i) = (b0 < -eps) ? -1.0 : 1.0;
    }
    /* 2. */
    const int status = ref_ranging_crash(Aa, m, na, bp, basis, 0, binv, xb);
    int kind = REF_CERT_NONE, index = -1;
    double value = NAN;
    if (status == REF_OPTIMAL) {
        int art = 0, viol = 0;
        for (int t = 0; t < m; ++t) {
            if (basis[t] >= n) {
                art = 1;
                continue;
            }
            const double L = lo[basis[t]], H = hi[basis[t]];
            if (xb[t] < L - eps || (H < INFINITY && xb[t] > H + eps)) viol = 1;
        }
        if (art) { /* 4. */
            for (int i = 0; i < m; ++i) {
                double u = 0.0;
                for (int t = 0; t < m; ++t)
                    if (basis[t] >= n) u = u + binv[(size_t)t * m + i];
                f[i] = -u;
            }
            double sum = 0.0;
            for (int i = 0; i < m; ++i)
                if (pos[n + i] >= 0) sum = sum + xb[pos[n + i]];
            int ok = sum > eps;
            for (int j = 0; j < n && ok; ++j) {
                if (pos[j] >= 0) continue;
                double g = 0.0;
                for (int i = 0; i < m; ++i) g = fma(f[i], AT(A, m, i, j), g);
                if (!bcert_sign_ok(g, at_upper[j], eps)) ok = 0;
            }
            if (ok) kind = REF_CERT_FARKAS;
        } else if (viol) { /* 5. */
            for (int t = 0; t < m && kind == REF_CERT_NONE; ++t) {
                const double L = lo[basis[t]], H = hi[basis[t]];
                const int below = xb[t] < L - eps, above = H < INFINITY && xb[t] > H + eps;
                if (!below && !above) continue;
                const double* br = binv + (size_t)t * m;
                int ok = 1;
                for (int j = 0; j < n && ok; ++j) {
                    if (pos[j] >= 0) continue;
                    double s = 0.0;
                    for (int i = 0; i < m; ++i) s = fma(br[i], AT(A, m, i, j), s);
                    if (!bcert_sign_ok(below ? s : -s, at_upper[j], eps)) ok = 0;
                }
                if (ok) {
                    kind = REF_CERT_FARKAS;
                    index = t;
                    for (int i = 0; i < m; ++i) f[i] = below ? br[i] : -br[i];
                }
            }
        } else { /* 6. */
            for (int j = 0; j < n && kind == REF_CERT_NONE; ++j) {
                if (pos[j] >= 0) continue;
                double d = c[j];
                int ok = 1;
                for (int t = 0; t < m; ++t) {
                    const double* br = binv + (size_t)t * m;
                    double s = 0.0;
                    for (int i = 0; i < m; ++i) s = fma(br[i], AT(A, m, i, j), s);
                    col[t] = s;
                    d = fma(-c[basis[t]], s, d);
                    if (!(s <= eps)) ok = 0;
                    if (!(s >= -eps) && hi[basis[t]] < INFINITY) ok = 0;
                }
                if (at_upper[j] || !(hi[j] == INFINITY)) ok = 0;
                if (ok && (maximize ? d > eps : d < -eps)) {
                    kind = REF_CERT_RAY;
                    index = j;
                    value = d;
                    for (int k = 0; k < n; ++k) ray_out[k] = 0.0;
                    ray_out[j] = 1.0;
                    for (int t = 0; t < m; ++t) ray_out[basis[t]] = -col[t];
                }
            }
        }
        if (kind == REF_CERT_FARKAS) {
            double s = 0.0;
            for (int i = 0; i < m; ++i) {
                farkas_out[i] = f[i];
                s = fma(bp[i], f[i], s);
            }
            if (index >= 0) {
                const double L = lo[basis[index]], H = hi[basis[index]];
                if (xb[index] < L - eps) {
                    if (L != 0.0) s = s - L;
                } else {
                    s = s + H;
                }
            }
            value = s;
        }
        *kind_out = kind;
        *value_out = value;
        *index_out = index;
    }
    free(col);
    free(f);
    free(xb);
    free(binv);
    free(Aa);
    free(bp);
    free(v);
    free(pos);
    return status;
}
