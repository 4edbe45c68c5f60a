/*
 * bounded_parametric_ref.c — TEST INFRASTRUCTURE ONLY: the parametric right-hand-side path and the parametric cost
 * path of a bounded-variable LP from an optimal basis and its at-upper flags (the lp_basis_bounded_parametric and
 * lp_basis_bounded_parametric_cost families).  Problem: A x = b, lo <= x <= hi, lo finite, hi finite or +inf; basis
 * (m, by position) and at_upper (n, 0/1) are what lp_simplex_bounded or its re-solve returned.  Stated on the slot
 * tableau of bounded_resolve_ref.c (included below: bref_t, bref_pivot's arithmetic, the complement, the crash of its
 * step 4), so that every step is one the kernels of basis_bounded_parametric.hip take with the same arithmetic.
 *
 * Both paths
 *   1. checks, in this order: a NULL output or max_breaks < 0 -> REF_BAD_ARG with nothing written; then every output
 *      is filled (nseg 0, NaN values, -1 indices and sides, the given basis and flags when they were passed); a NULL
 *      input or direction, m <= 0, n < m, t_max < 0 / NaN, eps < 0 / NaN, lo_j NaN or infinite, hi_j NaN, at_upper_j
 *      not 0 or 1 or 1 with hi_j = +inf, a basis index outside [0, n) -> REF_BAD_ARG; any hi_j < lo_j ->
 *      REF_INFEASIBLE.  Every outcome without a path (these, REF_SINGULAR, an invalid start) leaves that fill;
 *   2. tableau: bounded_resolve_ref.c steps 2-3 (x = lo + x', U_j = hi_j - lo_j, b' the fma chain over lo_j != 0 and
 *      then over the flagged columns, a flagged column held as -A_ij with cost -c_j);
 *   3. crash: bounded_resolve_ref.c step 4 over every stored row and column (skipped when the basic columns as
 *      loaded are the unit vectors in order and every cost row is zero there; a failure is REF_SINGULAR);
 *   4. start check: bounded_resolve_ref.c step 5 finds no violated position (xB_t < -eps below, U finite and
 *      U - xB_t < -eps above) and no slot of a variable < n with d > eps (max) / d < -eps (min), else REF_BAD_ARG
 *      (re-solve first);
 *   5. values in the caller's variables: position t holds variable k with tableau value v; w = up[k] ? U_k - v : v;
 *      x_t = lo_k == 0.0 ? w : lo_k + w.  A non-basic j is held at h_j = up[j] ? hi_j : lo_j.
 *
 * RHS path, z*(t) = opt { c.x : A x = b + t d, lo <= x <= hi }, one dual pivot per breakpoint
 *   R1. the tableau has W = n + 2 stored columns: slot n holds b' (beta after the crash), slot n + 1 holds d (delta),
 *       neither shifted nor complemented: the bounds do not move with t.  Rows 0..m;
 *   R2. segment k from t_k (t_0 = +0.0): positions t ascending; delta_t < -eps: tau = -beta_t / delta_t, the variable
 *       heads for its lower bound (of what the tableau holds; side = up[k]); delta_t > eps with U_N(t) finite:
 *       tau = (U_N(t) - beta_t) / delta_t, it heads for the other bound (side = !up[k]).  The breakpoint is the first
 *       strict minimum (a tie keeps the first position); t* = tau > t_k ? tau : t_k;
 *         - no candidate, or t* >= t_max: the path ends at t_max, REF_OPTIMAL, leave -1;
 *         - else r = the blocking position; blocked above, row r is read as if complemented (a = -T[r][s]).  The
 *           entering slot is bref_dual_loop's chain over row r: slots of a variable < n with a < -eps, q = d_s / a
 *           (max) or -d_s / a (min), the EPS-hysteresis chain (min) in variable order.  leave[k] = N(r), side[k];
 *         - no entering slot: the path ends at t*, REF_INFEASIBLE;
 *         - k == max_breaks: the path ends at t*, REF_ITER_LIMIT;
 *         - else, blocked above, the complement (row r's n slots negated, beta_r = U - beta_r, delta_r negated, the
 *           flag toggled); then the pivot over every slot, both right-hand columns and the cost row.  A blocking
 *           row that does not pivot leaves no trace: the returned basis and flags are the last segment's;
 *   R3. obj[k]: the chain s = fma(c_N(t), x_t, s) in position order from 0.0 with v = fma(t_k, delta_t, beta_t), then
 *       continued over the non-basic j ascending with h_j != 0.0 as s = fma(c_j, h_j, s) (the continuation of
 *       lp_basis_bounded_duals' w).  slope[k]: the chain s = fma(c_N(t), up ? -delta_t : delta_t, s).  For max z* is
 *       concave in t (slopes do not increase), for min convex (slopes do not decrease).
 *
 * Cost path, z*(t) = opt { (c + t g).x : A x = b, lo <= x <= hi }, one primal pivot or bound flip per breakpoint
 *   C1. W = n + 1 stored columns and two cost rows: row m holds c', row m + 1 holds g', each negated in the flagged
 *       columns; the crash prices both out (rows 0..m+1);
 *   C2. segment k from t_k: the slots of a variable < n in ascending variable order with delta_s > eps (max) or
 *       delta_s < -eps (min), tau = -d_s / delta_s; the first strict minimum; t* = tau > t_k ? tau : t_k;
 *         - no candidate, or t* >= t_max: the path ends at t_max, REF_OPTIMAL, enter -1;
 *         - else e enters by bounded_ref.c step 5's ratio test over its slot (the chain over the positions, theta the
 *           selected value); enter[k] = e;
 *         - no row and U_e = +inf: the path ends at t*, REF_UNBOUNDED;
 *         - else k == max_breaks: the path ends at t*, REF_ITER_LIMIT;
 *         - else no row or U_e <= theta: a BOUND FLIP: T[i][n] = fma(-U_e, T[i][se], T[i][n]) and the slot negated for
 *           i = 0 .. m+1, the flag toggled; recorded as a breakpoint with leave[k] = e and side[k] = the new flag;
 *         - else a pivot on row r over rows 0..m+1, the leaving variable complemented first when a_r < -eps (n slots
 *           of row r negated, xB_r = U - xB_r, the flag toggled); side[k] = the leaving variable's flag after that;
 *   C3. obj[k]: the chain of R3 with v = xB_t and the cost entry fma(t_k, g_j, c_j) in both parts; slope[k]: the same
 *       chain with g_j as the cost entry.  For max z* is convex in t (slopes do not decrease), for min concave.
 *
 * Outputs as parametric_ref.c step 5 (obj[nseg] by its step 4: the chain at the final end with the last basis; an end
 * at +inf gives obj[nseg-1] when the last slope is zero, else +inf or -inf by the slope's sign), and beside them
 * side (max_breaks + 1): the bound at which leave[k] stops, 0 lower, 1 upper, -1 where leave[k] is -1; at_upper_out
 * (n): the final flags.
 *
 * REQUIRED IDENTITY: with lo = 0, hi = +inf and no flag every output shared with ref_parametric / ref_parametric_cost
 * equals theirs bit for bit, side = 0 wherever leave >= 0 and at_upper_out = 0.  The chains above are written so that
 * it holds; should one of them, as written here, ever break it, the identity wins and the chain is what is wrong.
 *
 * Built with -ffp-contract=off (simplexmethod_amd/build.py: build_bounded_parametric_ref).  Only tests load it.
 */
#include "bounded_resolve_ref.c"

typedef struct {
    bref_t s;
    int rows;            /* m + 1 (RHS) or m + 2 (cost) */
    double *prow, *lcol;
    const double *lo, *hi, *c, *g;
} bpar_t;

static void bpar_fill(int m, int n, int max_breaks, const int* basis, const int* at_upper, double* t, double* obj,
                      double* slope, int* enter, int* leave, int* side, int* basis_out, int* at_upper_out) {
    for (int k = 0; k < max_breaks + 2; ++k) t[k] = obj[k] = NAN;
    for (int k = 0; k < max_breaks + 1; ++k) {
        slope[k] = NAN;
        enter[k] = leave[k] = side[k] = -1;
    }
    if (basis && m > 0) memcpy(basis_out, basis, sizeof(int) * (size_t)m);
    if (at_upper && n > 0) memcpy(at_upper_out, at_upper, sizeof(int) * (size_t)n);
}

/* bref_pivot's arithmetic over p->rows rows */
static void bpar_pivot(bpar_t* p, int r, int se) {
    bref_t* s = &p->s;
    const int W = s->W;
    double *prow = p->prow, *lcol = p->lcol;
    const double ur = TT(s, r, se);
    for (int j = 0; j < W; ++j) prow[j] = TT(s, r, j);
    for (int i = 0; i < p->rows; ++i) lcol[i] = (i == r) ? 1.0 / ur : -TT(s, i, se) / ur;
    for (int i = 0; i < p->rows; ++i)
        for (int j = 0; j < W; ++j) {
            const double l = lcol[i], pj = prow[j];
            TT(s, i, j) = (j == se) ? l : (i == r) ? pj * l : fma(l, pj, TT(s, i, j));
        }
    const int ve = s->slotvar[se], vl = s->basis[r];
    s->slotvar[se] = vl;
    s->basis[r] = ve;
    s->varslot[vl] = se;
    s->varslot[ve] = -1;
}

static void bpar_free(bpar_t* p) {
    bref_t* s = &p->s;
    free(p->lcol); free(p->prow); free(s->varslot); free(s->up); free(s->basis); free(s->slotvar); free(s->U);
    free(s->T);
}

/* steps 1 (the checks after the fill) to 4; REF_OPTIMAL leaves the installed tableau in *p, anything else frees it */
static int bpar_install(bpar_t* p, const double* A, int m, int n, const double* b, const double* c, const double* lo,
                        const double* hi, const int* N, const int* at_upper, int maximize, const double* dir,
                        int cost, double t_max, double eps) {
    if (m <= 0 || n < m || !A || !b || !c || !lo || !hi || !N || !at_upper || !dir) return REF_BAD_ARG;
    if (!(t_max >= 0.0) || !(eps >= 0.0)) return REF_BAD_ARG;
    for (int j = 0; j < n; ++j) {
        if (!isfinite(lo[j]) || isnan(hi[j])) return REF_BAD_ARG;
        if (at_upper[j] != 0 && at_upper[j] != 1) return REF_BAD_ARG;
        if (at_upper[j] && hi[j] == INFINITY) return REF_BAD_ARG;
    }
    for (int t = 0; t < m; ++t)
        if (N[t] < 0 || N[t] >= n) return REF_BAD_ARG;
    for (int j = 0; j < n; ++j)
        if (hi[j] < lo[j]) return REF_INFEASIBLE;

    bref_t* s = &p->s;
    const int rows = cost ? m + 2 : m + 1, W = cost ? n + 1 : n + 2, nv = n + m;
    p->rows = rows;
    p->lo = lo;
    p->hi = hi;
    p->c = c;
    p->g = cost ? dir : NULL;
    s->m = m;
    s->n = n;
    s->W = W;
    s->eps = eps;
    s->T = (double*)malloc(sizeof(double) * (size_t)rows * W);
    s->U = (double*)malloc(sizeof(double) * (size_t)nv);
    s->slotvar = (int*)malloc(sizeof(int) * (size_t)n);
    s->basis = (int*)malloc(sizeof(int) * (size_t)m);
    s->up = (int*)calloc((size_t)nv, sizeof(int));
    s->varslot = (int*)malloc(sizeof(int) * (size_t)nv);
    p->prow = (double*)malloc(sizeof(double) * (size_t)W);
    p->lcol = (double*)malloc(sizeof(double) * (size_t)rows);
    int* rowpos = (int*)malloc(sizeof(int) * (size_t)m);
    if (!s->T || !s->U || !s->slotvar || !s->basis || !s->up || !s->varslot || !p->prow || !p->lcol || !rowpos) abort();

    for (int j = 0; j < n; ++j) s->U[j] = hi[j] - lo[j], s->up[j] = at_upper[j];
    for (int k = n; k < nv; ++k) s->U[k] = INFINITY;
    for (int j = 0; j < n; ++j) s->slotvar[j] = j, s->varslot[j] = j;
    for (int t = 0; t < m; ++t) s->basis[t] = n + t, s->varslot[n + t] = -1;
    /* step 2 */
    for (int i = 0; i < m; ++i) {
        double acc = b[i];
        for (int j = 0; j < n; ++j)
            if (lo[j] != 0.0) acc = fma(-A[(size_t)j * m + i], lo[j], acc);
        for (int j = 0; j < n; ++j)
            if (s->up[j]) acc = fma(-A[(size_t)j * m + i], s->U[j], acc);
        for (int j = 0; j < n; ++j) {
            const double a = A[(size_t)j * m + i];
            TT(s, i, j) = s->up[j] ? -a : a;
        }
        TT(s, i, n) = acc;
        if (!cost) TT(s, i, n + 1) = dir[i];
    }
    for (int i = m; i < rows; ++i) {
        const double* cr = i == m ? c : dir;
        for (int j = 0; j < n; ++j) TT(s, i, j) = s->up[j] ? -cr[j] : cr[j];
        for (int j = n; j < W; ++j) TT(s, i, j) = 0.0;
    }

    /* step 3: the crash of bounded_resolve_ref.c step 4 over `rows` rows and W columns */
    int status = REF_OPTIMAL;
    int identity = 1;
    for (int t = 0; t < m && identity; ++t)
        for (int i = 0; i < m; ++i)
            if (TT(s, i, N[t]) != ((i == t) ? 1.0 : 0.0)) {
                identity = 0;
                break;
            }
    for (int t = 0; t < m && identity; ++t)
        for (int i = m; i < rows; ++i)
            if (TT(s, i, N[t]) != 0.0) identity = 0;
    if (identity) {
        for (int t = 0; t < m; ++t) {
            s->slotvar[N[t]] = n + t;
            s->varslot[n + t] = N[t];
            s->varslot[N[t]] = -1;
            s->basis[t] = N[t];
        }
    } else {
        double minp = INFINITY, maxp = 0.0;
        for (int t = 0; t < m; ++t) {
            const int q = N[t];
            int pr = -1;
            double big = -1.0;
            if (s->slotvar[q] == q)
                for (int i = 0; i < m; ++i) {
                    if (s->basis[i] < n) continue;
                    const double a = fabs(TT(s, i, q));
                    if (a > big) {
                        big = a;
                        pr = i;
                    }
                }
            if (!(big > 0.0)) {
                status = REF_SINGULAR;
                break;
            }
            if (big < minp) minp = big;
            if (big > maxp) maxp = big;
            bpar_pivot(p, pr, q);
            rowpos[t] = pr;
        }
        if (status == REF_OPTIMAL && minp <= DBL_EPSILON * (double)m * maxp) status = REF_SINGULAR;
        if (status == REF_OPTIMAL) {
            double* T2 = (double*)malloc(sizeof(double) * (size_t)rows * W);
            if (!T2) abort();
            for (int t = 0; t < m; ++t) memcpy(T2 + (size_t)t * W, s->T + (size_t)rowpos[t] * W, sizeof(double) * (size_t)W);
            memcpy(T2 + (size_t)m * W, s->T + (size_t)m * W, sizeof(double) * (size_t)(rows - m) * W);
            free(s->T);
            s->T = T2;
            for (int t = 0; t < m; ++t) s->basis[t] = N[t];
        }
    }
    free(rowpos);
    /* step 4 */
    if (status == REF_OPTIMAL) {
        for (int t = 0; t < m; ++t) {
            const double xb = TT(s, t, n), u = s->U[s->basis[t]];
            if (xb < -eps || (u < INFINITY && u - xb < -eps)) status = REF_BAD_ARG;
        }
        for (int sl = 0; sl < n; ++sl) {
            const double dj = TT(s, m, sl);
            if (s->slotvar[sl] < n && (maximize ? (dj > eps) : (dj < -eps))) status = REF_BAD_ARG;
        }
    }
    if (status != REF_OPTIMAL) bpar_free(p);
    return status;
}

/* step 5 */
static double bpar_x(const bpar_t* p, int k, double v) {
    const double w = p->s.up[k] ? p->s.U[k] - v : v;
    return p->lo[k] == 0.0 ? w : p->lo[k] + w;
}

/* R3 / C3: the value chain at tt (slope = 0) or the slope chain (slope = 1) */
static double bpar_chain(const bpar_t* p, double tt, int slope) {
    const bref_t* s = &p->s;
    const int m = s->m, n = s->n, cost = p->g != NULL;
    double z = 0.0;
    for (int t = 0; t < m; ++t) {
        const int k = s->basis[t];
        if (cost) {
            const double ce = slope ? p->g[k] : fma(tt, p->g[k], p->c[k]);
            z = fma(ce, bpar_x(p, k, TT(s, t, n)), z);
        } else if (slope) {
            const double de = TT(s, t, n + 1);
            z = fma(p->c[k], s->up[k] ? -de : de, z);
        } else {
            z = fma(p->c[k], bpar_x(p, k, fma(tt, TT(s, t, n + 1), TT(s, t, n))), z);
        }
    }
    if (!cost && slope) return z;
    for (int j = 0; j < n; ++j) {
        if (s->varslot[j] < 0) continue;
        const double h = s->up[j] ? p->hi[j] : p->lo[j];
        if (h == 0.0) continue;
        const double ce = !cost ? p->c[j] : slope ? p->g[j] : fma(tt, p->g[j], p->c[j]);
        z = fma(ce, h, z);
    }
    return z;
}

static void bpar_complement(bref_t* s, int r, int rhs) {
    const int n = s->n;
    for (int j = 0; j < n; ++j) TT(s, r, j) = -TT(s, r, j);
    TT(s, r, n) = s->U[s->basis[r]] - TT(s, r, n);
    if (rhs) TT(s, r, n + 1) = -TT(s, r, n + 1);
    s->up[s->basis[r]] ^= 1;
}

static int bpar_finish(bpar_t* p, int status, int k, double tend, int* nseg_out, double* t_out, double* obj_out,
                       const double* slope_out, int* basis_out, int* at_upper_out) {
    bref_t* s = &p->s;
    t_out[k + 1] = tend;
    if (tend == INFINITY)
        obj_out[k + 1] = slope_out[k] == 0.0 ? obj_out[k] : (slope_out[k] > 0.0 ? INFINITY : -INFINITY);
    else
        obj_out[k + 1] = bpar_chain(p, tend, 0);
    *nseg_out = k + 1;
    memcpy(basis_out, s->basis, sizeof(int) * (size_t)s->m);
    for (int j = 0; j < s->n; ++j) at_upper_out[j] = s->up[j];
    bpar_free(p);
    return status;
}

int ref_bounded_parametric(const double* A, int m, int n, const double* b, const double* c, const double* lo,
                           const double* hi, const int* basis, const int* at_upper, int maximize, const double* dir,
                           double t_max, double eps, int max_breaks, int* nseg_out, double* t_out, double* obj_out,
                           double* slope_out, int* enter_out, int* leave_out, int* side_out, int* basis_out,
                           int* at_upper_out) {
    if (!nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out || !side_out || !basis_out ||
        !at_upper_out || max_breaks < 0)
        return REF_BAD_ARG;
    *nseg_out = 0;
    bpar_fill(m, n, max_breaks, basis, at_upper, t_out, obj_out, slope_out, enter_out, leave_out, side_out, basis_out,
              at_upper_out);
    bpar_t P;
    bpar_t* p = &P;
    int status = bpar_install(p, A, m, n, b, c, lo, hi, basis, at_upper, maximize, dir, 0, t_max, eps);
    if (status != REF_OPTIMAL) return status;
    bref_t* s = &p->s;
    int k = 0;
    double tk = 0.0, tend;
    for (;;) {
        t_out[k] = tk;
        obj_out[k] = bpar_chain(p, tk, 0);
        slope_out[k] = bpar_chain(p, tk, 1);
        double best = 0.0;
        int r = -1, above = 0;
        for (int t = 0; t < m; ++t) {
            const double dl = TT(s, t, n + 1), u = s->U[s->basis[t]];
            double tau;
            int ab;
            if (dl < -eps) tau = -TT(s, t, n) / dl, ab = 0;
            else if (dl > eps && u < INFINITY) tau = (u - TT(s, t, n)) / dl, ab = 1;
            else continue;
            if (r < 0 || tau < best) {
                best = tau;
                r = t;
                above = ab;
            }
        }
        const double tstar = best > tk ? best : tk;
        if (r < 0 || tstar >= t_max) {
            tend = t_max;
            status = REF_OPTIMAL;
            break;
        }
        double qbest = INFINITY;
        int se = -1;
        for (int kk = 0; kk < n; ++kk) {
            const int sl = s->varslot[kk];
            if (sl < 0) continue;
            const double a = above ? -TT(s, r, sl) : TT(s, r, sl);
            if (!(a < -eps)) continue;
            const double q = maximize ? TT(s, m, sl) / a : -TT(s, m, sl) / a;
            if (q < qbest - eps) {
                qbest = q;
                se = sl;
            }
        }
        leave_out[k] = s->basis[r];
        side_out[k] = s->up[s->basis[r]] ^ above;
        tend = tstar;
        if (se < 0) { status = REF_INFEASIBLE; break; }
        if (k == max_breaks) { status = REF_ITER_LIMIT; break; }
        enter_out[k] = s->slotvar[se];
        if (above) bpar_complement(s, r, 1);
        bpar_pivot(p, r, se);
        ++k;
        tk = tstar;
    }
    enter_out[k] = -1;
    if (status == REF_OPTIMAL) leave_out[k] = side_out[k] = -1;
    return bpar_finish(p, status, k, tend, nseg_out, t_out, obj_out, slope_out, basis_out, at_upper_out);
}

int ref_bounded_parametric_cost(const double* A, int m, int n, const double* b, const double* c, const double* lo,
                                const double* hi, const int* basis, const int* at_upper, int maximize,
                                const double* g, double t_max, double eps, int max_breaks, int* nseg_out,
                                double* t_out, double* obj_out, double* slope_out, int* enter_out, int* leave_out,
                                int* side_out, int* basis_out, int* at_upper_out) {
    if (!nseg_out || !t_out || !obj_out || !slope_out || !enter_out || !leave_out || !side_out || !basis_out ||
        !at_upper_out || max_breaks < 0)
        return REF_BAD_ARG;
    *nseg_out = 0;
    bpar_fill(m, n, max_breaks, basis, at_upper, t_out, obj_out, slope_out, enter_out, leave_out, side_out, basis_out,
              at_upper_out);
    bpar_t P;
    bpar_t* p = &P;
    int status = bpar_install(p, A, m, n, b, c, lo, hi, basis, at_upper, maximize, g, 1, t_max, eps);
    if (status != REF_OPTIMAL) return status;
    bref_t* s = &p->s;
    int k = 0;
    double tk = 0.0, tend;
    for (;;) {
        t_out[k] = tk;
        obj_out[k] = bpar_chain(p, tk, 0);
        slope_out[k] = bpar_chain(p, tk, 1);
        double best = 0.0;
        int e = -1;
        for (int kk = 0; kk < n; ++kk) {
            const int sl = s->varslot[kk];
            if (sl < 0) continue;
            const double dl = TT(s, m + 1, sl);
            if (!(maximize ? (dl > eps) : (dl < -eps))) continue;
            const double tau = -TT(s, m, sl) / dl;
            if (e < 0 || tau < best) {
                best = tau;
                e = kk;
            }
        }
        const double tstar = best > tk ? best : tk;
        if (e < 0 || tstar >= t_max) {
            tend = t_max;
            status = REF_OPTIMAL;
            break;
        }
        const int se = s->varslot[e];
        double theta = INFINITY;
        int r = -1;
        for (int t = 0; t < m; ++t) {
            const double a = TT(s, t, se), xb = TT(s, t, n), u = s->U[s->basis[t]];
            const double v = (a > eps) ? xb / a : (a < -eps && u < INFINITY) ? (xb - u) / a : INFINITY;
            if (v < theta - eps) {
                theta = v;
                r = t;
            }
        }
        const double ue = s->U[e];
        enter_out[k] = e;
        tend = tstar;
        if (r < 0 && !(ue < INFINITY)) { status = REF_UNBOUNDED; break; }
        if (k == max_breaks) { status = REF_ITER_LIMIT; break; }
        if (r < 0 || ue <= theta) {
            for (int i = 0; i < p->rows; ++i) {
                TT(s, i, n) = fma(-ue, TT(s, i, se), TT(s, i, n));
                TT(s, i, se) = -TT(s, i, se);
            }
            s->up[e] ^= 1;
            leave_out[k] = e;
            side_out[k] = s->up[e];
        } else {
            if (TT(s, r, se) < -eps) bpar_complement(s, r, 0);
            leave_out[k] = s->basis[r];
            side_out[k] = s->up[s->basis[r]];
            bpar_pivot(p, r, se);
        }
        ++k;
        tk = tstar;
    }
    leave_out[k] = side_out[k] = -1;
    if (status == REF_OPTIMAL) enter_out[k] = -1;
    return bpar_finish(p, status, k, tend, nseg_out, t_out, obj_out, slope_out, basis_out, at_upper_out);
}
