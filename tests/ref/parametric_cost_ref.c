/*
 * parametric_cost_ref.c — TEST INFRASTRUCTURE ONLY: parametric cost analysis of an LP from an optimal basis (the
 * lp_basis_parametric_cost family), stated on the arithmetic of oracle/lp_oracle.c and of resolve_ref.c (included
 * below).  It walks z*(t) = opt { (c + t g)^T x : A x = b, x >= 0 } for t from 0 up to t_max, one primal pivot per
 * breakpoint.
 *
 *   1. tableau and crash: T = [A | b ; c | 0 ; g | 0], (m+2) x (n+1).  Row m holds the reduced costs d of c, row m+1
 *      the reduced costs delta of g.  The basis is installed with resolve_ref.c's crash over all m+2 rows (skipped
 *      only for the slack identity with c_B = 0 and g_B = 0; m Gauss-Jordan pivots with first-max partial pivoting
 *      over the unused rows, the singular verdict minp <= DBL_EPSILON*m*maxp, a repeated index ends as REF_SINGULAR,
 *      rows put in basis-position order).  A non-pivot row's new value depends only on itself and the pivot row, so
 *      the rows 0..m are bit-identical to the ones a crash on [A | b ; c | 0] gives for the same basis;
 *   2. start check: the basis must be primal feasible (no xB_t < -eps) and dual feasible at t = 0 (no non-basic
 *      j < n with d_j > eps for max, d_j < -eps for min), else REF_BAD_ARG (re-solve first);
 *   3. segment k (t_0 = +0.0) with the current basis: over non-basic j < n ascending with delta_j > eps (max) or
 *      delta_j < -eps (min), tau_j = -d_j / delta_j; the breakpoint is the first strict minimum (ranging_ref.c's
 *      take: a tie keeps the first index); t* = tau > t_k ? tau : t_k, so t never moves backwards.
 *        - no candidate, or t* >= t_max: the segment ends at t_max, status REF_OPTIMAL;
 *        - else e = the chosen column and the leaving position is tableau_loop's ratio test over column e
 *          (any_pos on !(u <= eps), ratios xB_i / u_i for u_i > eps, the EPS-hysteresis chain (min) in position
 *          order);
 *        - no leaving row: the LP is unbounded for every t > t*; the segment ends at t*, status REF_UNBOUNDED;
 *        - max_breaks pivots done already: the segment ends at t*, status REF_ITER_LIMIT;
 *        - else the oracle's tableau_pivot over all n+1 columns and both cost rows; t_{k+1} = t*; next segment;
 *   4. per segment k: obj[k] = sum_t fma(t_k, g[N_t], c[N_t]) * xB_t as the chain s = fma(cost, xB_t, s) in position
 *      order from s = 0.0; slope[k] = the chain s = fma(g[N_t], xB_t, s) in position order; enter[k] and leave[k]
 *      the variables of the pivot that ends the segment.  The last segment has leave -1 and enter the column that
 *      would enter (REF_UNBOUNDED, REF_ITER_LIMIT) or -1 (ended at t_max).  obj[nseg] is the chain at the final end
 *      with the last basis; an end at +inf gives obj[nseg-1] when the last slope is zero, else +inf or -inf by the
 *      slope's sign;
 *   5. outputs: as parametric_ref.c: nseg (1 .. max_breaks+1), t[0..nseg], obj[0..nseg], slope / enter / leave
 *      [0..nseg-1], the final basis by position.  Entries past the path are NaN (values) and -1 (indices).
 *      REF_SINGULAR and REF_BAD_ARG give nseg = 0, every entry NaN / -1 and the given basis back (when it was
 *      passed).
 *
 * REF_BAD_ARG also for: a NULL input or output, t_max < 0 / NaN, eps < 0 / NaN, max_breaks < 0, a basis index
 * outside [0, n).  A negative direction of t is -g.  Arrays: t_out / obj_out max_breaks+2, slope_out / enter_out /
 * leave_out max_breaks+1, basis_out m.  Built with -ffp-contract=off (simplexmethod_amd/build.py:
 * build_parametric_cost_ref).  Only tests load it.
 */
#include "resolve_ref.c"

static void fill_parametric_cost_nan(int m, int max_breaks, const int* basis, double* t, double* obj,
                                     double* slope, int* enter, int* leave, int* basis_out) {
    for (int k = 0; k < max_breaks + 2; ++k) {
        t[k] = NAN;
        obj[k] = NAN;
    }
    for (int k = 0; k < max_breaks + 1; ++k) {
        slope[k] = NAN;
        enter[k] = -1;
        leave[k] = -1;
    }
    if (basis) memcpy(basis_out, basis, sizeof(int) * (size_t)m);
}

/* sum_t fma(tk, g[N[t]], c[N[t]]) * xB_t (the chain in position order) */
static double cost_path_value(const double* T, int m, int n, int ld, const int* N, const double* c,
                              const double* g, double tk) {
    double s = 0.0;
    for (int t = 0; t < m; ++t) s = fma(fma(tk, g[N[t]], c[N[t]]), T[(size_t)t * ld + n], s);
    return s;
}

static double cost_path_slope(const double* T, int m, int n, int ld, const int* N, const double* g) {
    double s = 0.0;
    for (int t = 0; t < m; ++t) s = fma(g[N[t]], T[(size_t)t * ld + n], s);
    return s;
}

/* ranging_ref.c's take for a minimum */
static void take_min(double v, int k, double* bv, int* bk) {
    if (*bk < 0 || v < *bv || (v == *bv && k < *bk)) {
        *bv = v;
        *bk = k;
    }
}

int ref_parametric_cost(const double* A, int m, int n, const double* b, const double* c, const int* basis,
                        int maximize, const double* g, double t_max, double eps, int max_breaks, int* nseg_out,
                        double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out,
                        int* basis_out) {
    if (!nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out || !basis_out || max_breaks < 0)
        return REF_BAD_ARG;
    *nseg_out = 0;
    fill_parametric_cost_nan(m, max_breaks, basis, t_out, obj_out, slope_out, enter_out, leave_out, basis_out);
    if (m <= 0 || n < m || !A || !b || !c || !basis || !g) return REF_BAD_ARG;
    if (!(t_max >= 0.0) || !(eps >= 0.0)) return REF_BAD_ARG;
    for (int t = 0; t < m; ++t)
        if (basis[t] < 0 || basis[t] >= n) return REF_BAD_ARG;
    const int rows = m + 2, cols = n + 1, ld = cols;
    double* T = (double*)xmalloc(sizeof(double) * (size_t)rows * ld);
    int* N = (int*)xmalloc(sizeof(int) * (size_t)m);
    memcpy(N, basis, sizeof(int) * (size_t)m);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < n; ++j) T[(size_t)i * ld + j] = AT(A, m, i, j);
        T[(size_t)i * ld + n] = b[i];
    }
    for (int j = 0; j < n; ++j) {
        T[(size_t)m * ld + j] = c[j];
        T[(size_t)(m + 1) * ld + j] = g[j];
    }
    T[(size_t)m * ld + n] = 0.0;
    T[(size_t)(m + 1) * ld + n] = 0.0;

    /* 1. resolve_ref.c's crash over all m+2 rows */
    int status = REF_OPTIMAL;
    int identity = 1;
    for (int t = 0; t < m && identity; ++t)
        for (int i = 0; i < m; ++i)
            if (AT(A, m, i, N[t]) != ((i == t) ? 1.0 : 0.0)) { identity = 0; break; }
    for (int t = 0; t < m && identity; ++t)
        if (c[N[t]] != 0.0 || g[N[t]] != 0.0) identity = 0;
    if (!identity) {
        int* rowpos = (int*)xmalloc(sizeof(int) * (size_t)m);
        unsigned char* used = (unsigned char*)xmalloc((size_t)m);
        memset(used, 0, (size_t)m);
        double minp = INFINITY, maxp = 0.0;
        for (int t = 0; t < m; ++t) {
            const int q = N[t];
            int p = -1;
            double big = -1.0;
            for (int i = 0; i < m; ++i) {
                if (used[i]) continue;
                double a = fabs(T[(size_t)i * ld + q]);
                if (a > big) { big = a; p = i; }
            }
            if (!(big > 0.0)) { status = REF_SINGULAR; break; }
            if (big < minp) minp = big;
            if (big > maxp) maxp = big;
            tableau_pivot(T, rows, cols, ld, p, q);
            used[p] = 1;
            rowpos[t] = p;
        }
        if (status == REF_OPTIMAL && minp <= DBL_EPSILON * (double)m * maxp) status = REF_SINGULAR;
        if (status == REF_OPTIMAL) {
            double* T2 = (double*)xmalloc(sizeof(double) * (size_t)rows * ld);
            for (int t = 0; t < m; ++t)
                memcpy(T2 + (size_t)t * ld, T + (size_t)rowpos[t] * ld, sizeof(double) * (size_t)ld);
            memcpy(T2 + (size_t)m * ld, T + (size_t)m * ld, sizeof(double) * 2 * (size_t)ld);
            free(T);
            T = T2;
        }
        free(used);
        free(rowpos);
    }
    unsigned char* nonbasic = (unsigned char*)xmalloc((size_t)n);
    unsigned char* rowmask = (unsigned char*)xmalloc((size_t)m);
    double* ratio = (double*)xmalloc(sizeof(double) * (size_t)m);
    /* 2. start check */
    if (status == REF_OPTIMAL) {
        nonbasic_flags(nonbasic, N, m, n);
        const double* d = T + (size_t)m * ld;
        for (int t = 0; t < m; ++t)
            if (T[(size_t)t * ld + n] < -eps) status = REF_BAD_ARG;
        for (int j = 0; j < n; ++j)
            if (nonbasic[j] && (maximize ? (d[j] > eps) : (d[j] < -eps))) status = REF_BAD_ARG;
    }
    if (status != REF_OPTIMAL) {
        free(ratio); free(rowmask); free(nonbasic); free(N); free(T);
        return status;
    }
    /* 3. and 4. the segments */
    int k = 0;
    double tk = 0.0, tend;
    for (;;) {
        t_out[k] = tk;
        obj_out[k] = cost_path_value(T, m, n, ld, N, c, g, tk);
        slope_out[k] = cost_path_slope(T, m, n, ld, N, g);
        nonbasic_flags(nonbasic, N, m, n);
        const double* d = T + (size_t)m * ld;
        const double* dl = T + (size_t)(m + 1) * ld;
        double best = 0.0;
        int e = -1;
        for (int j = 0; j < n; ++j) {
            if (!nonbasic[j] || !(maximize ? (dl[j] > eps) : (dl[j] < -eps))) continue;
            take_min(-d[j] / dl[j], j, &best, &e);
        }
        const double tstar = best > tk ? best : tk;
        if (e < 0 || tstar >= t_max) {
            tend = t_max;
            status = REF_OPTIMAL;
            break;
        }
        int any_pos = 0;
        for (int i = 0; i < m; ++i) {
            const double ui = T[(size_t)i * ld + e];
            if (!(ui <= eps)) any_pos = 1;
            rowmask[i] = (ui > eps);
            ratio[i] = rowmask[i] ? T[(size_t)i * ld + n] / ui : 0.0;
        }
        const int r = any_pos ? chain_select(ratio, rowmask, m, 0, eps) : -1;
        enter_out[k] = e;
        tend = tstar;
        if (r < 0) { status = REF_UNBOUNDED; break; }
        if (k == max_breaks) { status = REF_ITER_LIMIT; break; }
        leave_out[k] = N[r];
        N[r] = e;
        tableau_pivot(T, rows, cols, ld, r, e);
        ++k;
        tk = tstar;
    }
    leave_out[k] = -1;
    if (status == REF_OPTIMAL) enter_out[k] = -1;
    t_out[k + 1] = tend;
    if (tend == INFINITY)
        obj_out[k + 1] = slope_out[k] == 0.0 ? obj_out[k] : (slope_out[k] > 0.0 ? INFINITY : -INFINITY);
    else
        obj_out[k + 1] = cost_path_value(T, m, n, ld, N, c, g, tend);
    *nseg_out = k + 1;
    memcpy(basis_out, N, sizeof(int) * (size_t)m);
    free(ratio); free(rowmask); free(nonbasic); free(N); free(T);
    return status;
}
