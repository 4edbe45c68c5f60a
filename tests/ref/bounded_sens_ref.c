/*
 * bounded_sens_ref.c — TEST INFRASTRUCTURE ONLY: the dual solution and RHS / cost ranging of a bounded-variable LP
 * (opt c.x, A x = b, lo <= x <= hi, lo finite, hi finite or +inf) at a given basis and given at-upper flags: the
 * lp_basis_bounded_duals / lp_basis_bounded_ranging family.  Everything is stated in the caller's original variables
 * (no shift, no complemented column, no slot tableau) on the arithmetic of duals_ref.c and ranging_ref.c:
 *
 *   1. checks, as bounded_resolve_ref.c: lo_j NaN or infinite, hi_j NaN, at_upper[j] not 0 or 1, or 1 with
 *      hi_j = +inf, basis[t] outside [0, n), for ranging eps < 0 or NaN -> REF_BAD_ARG.  Any hi_j < lo_j ->
 *      REF_INFEASIBLE;
 *   2. held values: a non-basic column sits at v_j = hi_j if at_upper[j], else lo_j.  The flag of a basic column is
 *      not read (the solver may return a basic column held complemented; in original variables that changes nothing);
 *   3. b': per row i the chain acc = fma(-A[i][j], v_j, acc) from acc = b_i over the non-basic j ascending with
 *      v_j != 0.0;
 *   4. Binv and xB: ref_ranging_crash on [B | I | b'] (explicit form).  x[basis[t]] = xB[t], x[j] = v_j for non-basic j;
 *   5. y, d: exactly ref_duals(A, b, c, basis): basic d is exactly 0.0;
 *   6. w: the chain s = fma(b_i, y_i, s) from 0 over i ascending, continued over the non-basic j ascending with
 *      v_j != 0.0 as s = fma(d_j, v_j, s).  At an optimal basis w = c.x.  Optimal (not checked here) means, under max,
 *      d_j <= eps at a lower bound and d_j >= -eps at an upper bound; under min the signs are the other way round;
 *   7. RHS range of row i: beta_t = Binv[t][i], L_t = lo[basis[t]], H_t = hi[basis[t]], nL = (L_t == 0.0) ? -xB[t]
 *      : L_t - xB[t], nH = H_t - xB[t].  Over t ascending, beta_t > eps: nL / beta_t is a candidate of the lower end and,
 *      H_t finite, nH / beta_t one of the upper end; beta_t < -eps: nL / beta_t goes to the upper end and, H_t finite,
 *      nH / beta_t to the lower end.  Lower end = max, upper end = min, the first t wins a tie and its own value is
 *      reported: out b_i + delta, the leaving variable basis[t] and its side (0: it leaves at its lower bound, 1: at
 *      its upper bound); an empty side -inf / +inf, -1 and -1;
 *   8. cost ranges: the sense of a non-basic j is mx_j = maximize XOR at_upper[j]: [-inf, c_j - d_j] if mx_j, else
 *      [c_j - d_j, +inf] (the finite end carries j, the infinite end -1).  Basic column basis[t]: alpha[t][j] =
 *      sum_i Binv[t][i] A[i][j] as one fma chain in row order from 0, over the non-basic j ascending with
 *      |alpha| > eps, rho = d_j / alpha: a lower-end candidate (max) if (alpha > eps) == mx_j, else an upper-end
 *      candidate (min); the first j wins a tie; out c + delta and j;
 *   9. outputs in interleaved pairs as ranging_ref.c ([2k] lower end, [2k+1] upper end); NaN values and -1 indices
 *      and sides whenever the status is not REF_OPTIMAL (REF_SINGULAR when either crash is singular).
 *
 * With lo = 0, hi = +inf and no flag steps 3-6 give ref_duals's y, d, w and steps 7-8 ref_ranging's ends and indices
 * bit for bit, and every side is 0 or -1.  Built with -ffp-contract=off (simplexmethod_amd/build.py:
 * build_bounded_sens_ref).  Only tests load it.
 */
#include "ranging_ref.c"

enum { REF_INFEASIBLE = 4 };

static void bsens_fill_duals(int m, int n, double* x, double* y, double* d, double* w) {
    for (int j = 0; j < n; ++j) x[j] = d[j] = NAN;
    for (int t = 0; t < m; ++t) y[t] = NAN;
    *w = NAN;
}

static void bsens_fill_ranging(int m, int n, double* rhs, int* rhs_var, int* rhs_side, double* cost, int* cost_var) {
    fill_ranging_nan(m, n, rhs, rhs_var, cost, cost_var);
    for (int k = 0; k < 2 * m; ++k) rhs_side[k] = -1;
}

/* step 1 */
static int bsens_check(int m, int n, const double* lo, const double* hi, const int* basis, const int* at_upper) {
    for (int j = 0; j < n; ++j) {
        if (!isfinite(lo[j]) || isnan(hi[j])) return REF_BAD_ARG;
        if (at_upper[j] != 0 && at_upper[j] != 1) return REF_BAD_ARG;
        if (at_upper[j] && hi[j] == INFINITY) return REF_BAD_ARG;
    }
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) return REF_BAD_ARG;
    for (int j = 0; j < n; ++j)
        if (hi[j] < lo[j]) return REF_INFEASIBLE;
    return REF_OPTIMAL;
}

/* steps 2-4: basic (n flags), v (n, 0.0 for basic columns), Binv (m x m), xB (m) */
static int bsens_point(const double* A, int m, int n, const double* b, const double* lo, const double* hi,
                       const int* basis, const int* at_upper, unsigned char* basic, double* v, double* binv,
                       double* xb) {
    memset(basic, 0, (size_t)n);
    for (int t = 0; t < m; ++t) basic[basis[t]] = 1;
    for (int j = 0; j < n; ++j) v[j] = basic[j] ? 0.0 : at_upper[j] ? hi[j] : lo[j];
    double* bp = (double*)xmalloc(sizeof(double) * (size_t)m);
    for (int i = 0; i < m; ++i) {
        double acc = b[i];
        for (int j = 0; j < n; ++j)
            if (!basic[j] && v[j] != 0.0) acc = fma(-AT(A, m, i, j), v[j], acc);
        bp[i] = acc;
    }
    const int status = ref_ranging_crash(A, m, n, bp, basis, 0, binv, xb);
    free(bp);
    return status;
}

int ref_bounded_duals(const double* A, int m, int n, const double* b, const double* c, const double* lo,
                      const double* hi, const int* basis, const int* at_upper, double* x_out, double* y_out,
                      double* d_out, double* w_out) {
    if (m <= 0 || n < m || !A || !b || !c || !lo || !hi || !basis || !at_upper) return REF_BAD_ARG;
    if (!x_out || !y_out || !d_out || !w_out) return REF_BAD_ARG;
    bsens_fill_duals(m, n, x_out, y_out, d_out, w_out);
    int status = bsens_check(m, n, lo, hi, basis, at_upper);
    if (status != REF_OPTIMAL) return status;
    unsigned char* basic = (unsigned char*)xmalloc((size_t)n);
    double* v = (double*)xmalloc(sizeof(double) * (size_t)n);
    double* binv = (double*)xmalloc(sizeof(double) * (size_t)m * m);
    double* xb = (double*)xmalloc(sizeof(double) * (size_t)m);
    double* y = (double*)xmalloc(sizeof(double) * (size_t)m);
    double* d = (double*)xmalloc(sizeof(double) * (size_t)n);
    double w;
    status = bsens_point(A, m, n, b, lo, hi, basis, at_upper, basic, v, binv, xb);
    if (status == REF_OPTIMAL) status = ref_duals(A, m, n, b, c, basis, y, d, &w);
    if (status == REF_OPTIMAL) {
        for (int j = 0; j < n; ++j) x_out[j] = v[j];
        for (int t = 0; t < m; ++t) x_out[basis[t]] = xb[t];
        memcpy(y_out, y, sizeof(double) * (size_t)m);
        memcpy(d_out, d, sizeof(double) * (size_t)n);
        double s = w;   /* 6.: ref_duals's chain over the rows, continued over the held non-basic columns */
        for (int j = 0; j < n; ++j)
            if (!basic[j] && v[j] != 0.0) s = fma(d[j], v[j], s);
        *w_out = s;
    }
    free(d);
    free(y);
    free(xb);
    free(binv);
    free(v);
    free(basic);
    return status;
}

int ref_bounded_ranging(const double* A, int m, int n, const double* b, const double* c, const double* lo,
                        const double* hi, const int* basis, const int* at_upper, int maximize, double eps,
                        double* rhs_out, int* rhs_var_out, int* rhs_side_out, double* cost_out, int* cost_var_out) {
    if (m <= 0 || n < m || !A || !b || !c || !lo || !hi || !basis || !at_upper) return REF_BAD_ARG;
    if (!rhs_out || !rhs_var_out || !rhs_side_out || !cost_out || !cost_var_out) return REF_BAD_ARG;
    bsens_fill_ranging(m, n, rhs_out, rhs_var_out, rhs_side_out, cost_out, cost_var_out);
    if (!(eps >= 0.0)) return REF_BAD_ARG;
    int status = bsens_check(m, n, lo, hi, basis, at_upper);
    if (status != REF_OPTIMAL) return status;
    unsigned char* basic = (unsigned char*)xmalloc((size_t)n);
    double* v = (double*)xmalloc(sizeof(double) * (size_t)n);
    double* binv = (double*)xmalloc(sizeof(double) * (size_t)m * m);
    double* xb = (double*)xmalloc(sizeof(double) * (size_t)m);
    double* y = (double*)xmalloc(sizeof(double) * (size_t)m);
    double* d = (double*)xmalloc(sizeof(double) * (size_t)n);
    double w;
    status = bsens_point(A, m, n, b, lo, hi, basis, at_upper, basic, v, binv, xb);
    if (status == REF_OPTIMAL) status = ref_duals(A, m, n, b, c, basis, y, d, &w);
    if (status == REF_OPTIMAL) {
        for (int i = 0; i < m; ++i) {   /* 7. */
            double dl = 0.0, dh = 0.0;
            int kl = -1, kh = -1, sl = -1, sh = -1;
            for (int t = 0; t < m; ++t) {
                const double beta = binv[(size_t)t * m + i];
                const double L = lo[basis[t]], H = hi[basis[t]];
                const double nL = (L == 0.0) ? -xb[t] : L - xb[t], nH = H - xb[t];
                if (beta > eps) {
                    int k0 = kl;
                    take(nL / beta, t, 1, &dl, &kl);
                    if (kl != k0) sl = 0;
                    if (H < INFINITY) {
                        k0 = kh;
                        take(nH / beta, t, 0, &dh, &kh);
                        if (kh != k0) sh = 1;
                    }
                } else if (beta < -eps) {
                    int k0 = kh;
                    take(nL / beta, t, 0, &dh, &kh);
                    if (kh != k0) sh = 0;
                    if (H < INFINITY) {
                        k0 = kl;
                        take(nH / beta, t, 1, &dl, &kl);
                        if (kl != k0) sl = 1;
                    }
                }
            }
            rhs_out[2 * i] = kl < 0 ? -INFINITY : b[i] + dl;
            rhs_out[2 * i + 1] = kh < 0 ? INFINITY : b[i] + dh;
            rhs_var_out[2 * i] = kl < 0 ? -1 : basis[kl];
            rhs_var_out[2 * i + 1] = kh < 0 ? -1 : basis[kh];
            rhs_side_out[2 * i] = sl;
            rhs_side_out[2 * i + 1] = sh;
        }
        for (int j = 0; j < n; ++j) {   /* 8., non-basic */
            if (basic[j]) continue;
            const int mx = (maximize != 0) != (at_upper[j] != 0);
            const double e = c[j] - d[j];
            cost_out[2 * j] = mx ? -INFINITY : e;
            cost_out[2 * j + 1] = mx ? e : INFINITY;
            cost_var_out[2 * j] = mx ? -1 : j;
            cost_var_out[2 * j + 1] = mx ? j : -1;
        }
        for (int t = 0; t < m; ++t) {   /* 8., basic */
            double dl = 0.0, dh = 0.0;
            int kl = -1, kh = -1;
            const double* br = binv + (size_t)t * m;
            for (int j = 0; j < n; ++j) {
                if (basic[j]) continue;
                double s = 0.0;
                for (int i = 0; i < m; ++i) s = fma(br[i], AT(A, m, i, j), s);
                if (!(s > eps) && !(s < -eps)) continue;
                const int mx = (maximize != 0) != (at_upper[j] != 0);
                if ((s > eps) == mx) take(d[j] / s, j, 1, &dl, &kl);
                else take(d[j] / s, j, 0, &dh, &kh);
            }
            const int q = basis[t];
            cost_out[2 * q] = kl < 0 ? -INFINITY : c[q] + dl;
            cost_out[2 * q + 1] = kh < 0 ? INFINITY : c[q] + dh;
            cost_var_out[2 * q] = kl;
            cost_var_out[2 * q + 1] = kh;
        }
    }
    free(d);
    free(y);
    free(xb);
    free(binv);
    free(v);
    free(basic);
    return status;
}
