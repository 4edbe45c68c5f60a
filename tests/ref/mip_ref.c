/*
 * mip_ref.c — TEST INFRASTRUCTURE ONLY: depth-first branch-and-bound for an integer LP (the lp_mip_solve family),
 * stated on the arithmetic of resolve_ref.c (included below).  Problem: opt c.x, A x = b, x >= 0, x_j integral for
 * every j with integer[j] = 1 (j < n_orig).
 *
 *   1. root: ref_resolve's crash (skipped for the slack identity with zero costs), classification and loop, so a
 *      root result is lp_simplex_resolve's bit for bit;
 *   2. a node LP optimum: x from the basis (x_{N_t} = xB_t, zeros elsewhere), z = sum_{j<n} c_j x_j in index order
 *      (no fma).  With an incumbent z*, the node is pruned unless it beats z* by more than gap (max: z > z* + gap,
 *      min: z < z* - gap).  Else the branching variable is the marked j < n_orig of largest min(f, 1-f),
 *      f = x_j - floor(x_j), among those with min(f, 1-f) > int_tol, ties to the lowest index; none: the node is the
 *      new incumbent.  A fractional node with max_depth branch rows is abandoned;
 *   3. branching at a node with L branch rows (level L) records (j, v = x_j, z, the first side, the node's basis)
 *      and appends one row and one slack column, variable n + L.  Down: x_j + s = floor(v); up: -x_j + s = -ceil(v).
 *      The side nearer to v goes first (down when f <= 0.5).  The tableau grows to (m+L+1) rows and (n+L+1)
 *      columns: the rhs column and the cost row move out by one;
 *   4. first child (dive): the row is appended in tableau form to the parent's final tableau: -T[t][k] (down) or
 *      +T[t][k] (up) for the non-basic k, 0 for the basic columns, 1 in the slack's column, rhs floor(v) - v or
 *      v - ceil(v), where t is x_j's basis position; the slack is basic there.  Then the dual loop;
 *   5. second child (rebuild): T = [A | 0 | b] plus the branch rows of the path, the parent's basis plus the new
 *      slack installed by the crash (never skipped), then the root's classification and loop;
 *   6. a node LP solve is counted before it starts: with max_nodes solved, the search stops (LP_ITER_LIMIT).  A node
 *      that hits max_iter stops the search (LP_ITER_LIMIT); one that ends LP_SINGULAR, LP_BAD_ARG or LP_UNBOUNDED
 *      stops it with that status;
 *   7. bound: the best of the incumbent and the open or abandoned nodes (a pending second child and an interrupted
 *      node carry their parent's z); when that best does not beat z* by more than gap, z*.  No incumbent and none
 *      open: NaN.  A complete search is REF_OPTIMAL with an incumbent, REF_INFEASIBLE without, and REF_ITER_LIMIT
 *      when an abandoned node beats the incumbent by more than gap (or there is no incumbent).  A root that is not
 *      optimal gives its status: bound +-inf for REF_UNBOUNDED and REF_ITER_LIMIT, NaN otherwise.
 *
 * stats_out[4]: nodes solved (the root included), dual pivots, primal pivots, deepest level solved.  Crash pivots are
 * not counted.  Built with -ffp-contract=off (simplexmethod_amd/build.py: build_mip_ref).  Only tests load it.
 */
#include "resolve_ref.c"

#define MIP_MAX_DEPTH 64

/* the crash of ref_resolve over an (mm+1) x (nn+1) tableau with row pitch ld: m forced pivots, the singular
 * verdict, rows into basis-position order */
static int mip_crash(double* T, int mm, int nn, int ld, const int* N) {
    const int rows = mm + 1, cols = nn + 1;
    int status = REF_OPTIMAL;
    int* rowpos = (int*)xmalloc(sizeof(int) * (size_t)mm);
    unsigned char* used = (unsigned char*)xmalloc((size_t)mm);
    memset(used, 0, (size_t)mm);
    double minp = INFINITY, maxp = 0.0;
    for (int t = 0; t < mm; ++t) {
        const int q = N[t];
        int p = -1;
        double big = -1.0;
        for (int i = 0; i < mm; ++i) {
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
    if (status == REF_OPTIMAL && minp <= DBL_EPSILON * (double)mm * maxp) status = REF_SINGULAR;
    if (status == REF_OPTIMAL) {
        double* T2 = (double*)xmalloc(sizeof(double) * (size_t)mm * ld);
        for (int t = 0; t < mm; ++t)
            memcpy(T2 + (size_t)t * ld, T + (size_t)rowpos[t] * ld, sizeof(double) * (size_t)ld);
        memcpy(T, T2, sizeof(double) * (size_t)mm * ld);
        free(T2);
    }
    free(used);
    free(rowpos);
    return status;
}

/* classification and the matching loop (ref_resolve's) after an install */
static int mip_classify_run(double* T, int mm, int nn, int ld, int* N, int maximize, double eps, int max_iter,
                            int* itd, int* itp) {
    int primal_feasible = 1, dual_feasible = 1;
    for (int t = 0; t < mm; ++t)
        if (T[(size_t)t * ld + nn] < -eps) primal_feasible = 0;
    unsigned char* nonbasic = (unsigned char*)xmalloc((size_t)nn);
    nonbasic_flags(nonbasic, N, mm, nn);
    const double* d = T + (size_t)mm * ld;
    for (int j = 0; j < nn; ++j)
        if (nonbasic[j] && (maximize ? (d[j] > eps) : (d[j] < -eps))) dual_feasible = 0;
    free(nonbasic);
    int it = 0, st = REF_BAD_ARG;   /* max_iter bounds each node's pivots */
    if (primal_feasible) {
        st = primal_loop(T, mm, nn, ld, N, maximize, eps, max_iter, &it, NULL, NULL, 0);
        *itp += it;
    } else if (dual_feasible) {
        st = dual_loop(T, mm, nn, ld, N, maximize, eps, max_iter, &it, NULL, NULL, 0);
        *itd += it;
    }
    return st;
}

typedef struct {
    int j, first_down, second_taken;
    double v, z;
    int* basis; /* the node's basis, m + level entries, and room for the new slack */
} mip_record;

static int mip_beats(double z, double zs, int maximize, double gap) {
    return maximize ? (z > zs + gap) : (z < zs - gap);
}

int ref_mip(const double* A, int m, int n, const double* b, const double* c, const int* basis_in, int maximize,
            int n_orig, const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes,
            int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out) {
    if (m <= 0 || n < m || !A || !b || !c || !basis_in || !integer) return REF_BAD_ARG;
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out) return REF_BAD_ARG;
    if (n_orig <= 0 || n_orig > n) return REF_BAD_ARG;
    if (max_depth < 0 || max_depth > MIP_MAX_DEPTH || max_nodes < 1) return REF_BAD_ARG;
    if (!(int_tol >= 0.0 && int_tol < 0.5) || !(gap >= 0.0)) return REF_BAD_ARG;
    for (int t = 0; t < m; ++t)
        if (basis_in[t] < 0 || basis_in[t] >= n) return REF_BAD_ARG;
    for (int j = 0; j < n; ++j)
        if ((integer[j] != 0 && integer[j] != 1) || (integer[j] && j >= n_orig)) return REF_BAD_ARG;

    const int D = max_depth, ld = n + D + 1;
    double* T = (double*)xmalloc(sizeof(double) * (size_t)(m + D + 1) * ld);
    int* N = (int*)xmalloc(sizeof(int) * (size_t)(m + D));
    double* x = (double*)xmalloc(sizeof(double) * (size_t)(n + D));
    mip_record rec[MIP_MAX_DEPTH];
    for (int k = 0; k < D; ++k) rec[k].basis = (int*)xmalloc(sizeof(int) * (size_t)(m + k + 1));
    int stats[4] = {0, 0, 0, 0};
    for (int j = 0; j < n_orig; ++j) x_out[j] = NAN;
    *obj_out = NAN;
    *bound_out = NAN;
    *found_out = 0;

    /* ---- root: ref_resolve's install */
    memcpy(N, basis_in, sizeof(int) * (size_t)m);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < n; ++j) T[(size_t)i * ld + j] = AT(A, m, i, j);
        T[(size_t)i * ld + n] = b[i];
    }
    for (int j = 0; j < n; ++j) T[(size_t)m * ld + j] = c[j];
    T[(size_t)m * ld + n] = 0.0;
    int identity = 1;
    for (int t = 0; t < m && identity; ++t)
        for (int i = 0; i < m; ++i)
            if (AT(A, m, i, N[t]) != ((i == t) ? 1.0 : 0.0)) { identity = 0; break; }
    for (int t = 0; t < m && identity; ++t)
        if (c[N[t]] != 0.0) identity = 0;
    int st = identity ? REF_OPTIMAL : mip_crash(T, m, n, ld, N);
    if (st == REF_OPTIMAL) st = mip_classify_run(T, m, n, ld, N, maximize, eps, max_iter, &stats[1], &stats[2]);
    stats[0] = 1;

    int status = st;
    if (st != REF_OPTIMAL) {
        if (st == REF_UNBOUNDED || st == REF_ITER_LIMIT) *bound_out = maximize ? INFINITY : -INFINITY;
    } else {
        int L = 0, top = -1, found = 0, stop = REF_OPTIMAL, have_ab = 0;
        double zstar = 0.0, zab = 0.0;
        for (;;) {
            const int mm = m + L, nn = n + L;
            int backtrack = 1;
            if (st == REF_OPTIMAL) {
                for (int j = 0; j < nn; ++j) x[j] = 0.0;
                for (int t = 0; t < mm; ++t) x[N[t]] = T[(size_t)t * ld + nn];
                double z = 0.0;
                for (int j = 0; j < n; ++j) z += c[j] * x[j];
                if (!found || mip_beats(z, zstar, maximize, gap)) {
                    int jb = -1;
                    double dbest = 0.0;
                    for (int j = 0; j < n_orig; ++j) {
                        if (!integer[j]) continue;
                        const double f = x[j] - floor(x[j]);
                        const double dist = f < 1.0 - f ? f : 1.0 - f;
                        if (dist > int_tol && dist > dbest) { dbest = dist; jb = j; }
                    }
                    if (jb < 0) {
                        found = 1;
                        zstar = z;
                        for (int j = 0; j < n_orig; ++j) x_out[j] = x[j];
                    } else if (L == D) {
                        if (!have_ab || mip_beats(z, zab, maximize, 0.0)) zab = z;
                        have_ab = 1;
                    } else {
                        /* ---- branch: record level L, then the first child by appending the row */
                        mip_record* R = &rec[L];
                        const double v = x[jb];
                        R->j = jb;
                        R->v = v;
                        R->z = z;
                        R->first_down = (v - floor(v)) <= 0.5;
                        R->second_taken = 0;
                        memcpy(R->basis, N, sizeof(int) * (size_t)mm);
                        top = L;
                        if (stats[0] >= max_nodes) { stop = REF_ITER_LIMIT; break; }
                        int t = 0;
                        while (N[t] != jb) ++t;
                        /* rhs column nn -> nn+1, the cost row mm -> mm+1 */
                        for (int i = 0; i <= mm; ++i) {
                            T[(size_t)i * ld + nn + 1] = T[(size_t)i * ld + nn];
                            T[(size_t)i * ld + nn] = 0.0;
                        }
                        memcpy(T + (size_t)(mm + 1) * ld, T + (size_t)mm * ld, sizeof(double) * (size_t)(nn + 2));
                        double* Rw = T + (size_t)mm * ld;
                        const double* Tt = T + (size_t)t * ld;
                        for (int k = 0; k < nn; ++k) Rw[k] = R->first_down ? -Tt[k] : Tt[k];
                        for (int q = 0; q < mm; ++q) Rw[N[q]] = 0.0;
                        Rw[nn] = 1.0;
                        Rw[nn + 1] = R->first_down ? floor(v) - v : v - ceil(v);
                        N[mm] = nn;
                        ++L;
                        ++stats[0];
                        if (L > stats[3]) stats[3] = L;
                        int itd = 0;
                        st = dual_loop(T, m + L, n + L, ld, N, maximize, eps, max_iter, &itd, NULL, NULL, 0);
                        stats[1] += itd;
                        backtrack = 0;
                    }
                }
            } else if (st != REF_INFEASIBLE) {
                stop = st;
                break;
            }
            if (!backtrack) continue;
            while (top >= 0 && rec[top].second_taken) --top;
            if (top < 0) break;
            rec[top].second_taken = 1;
            if (stats[0] >= max_nodes) { stop = REF_ITER_LIMIT; break; }
            /* ---- the second child of record `top`, rebuilt from A and the branch rows of its path */
            L = top + 1;
            const int mm2 = m + L, nn2 = n + L;
            for (int i = 0; i <= mm2; ++i)
                for (int j = 0; j <= nn2; ++j) T[(size_t)i * ld + j] = 0.0;
            for (int i = 0; i < m; ++i) {
                for (int j = 0; j < n; ++j) T[(size_t)i * ld + j] = AT(A, m, i, j);
                T[(size_t)i * ld + nn2] = b[i];
            }
            for (int l = 0; l < L; ++l) {
                const int down = rec[l].second_taken ? !rec[l].first_down : rec[l].first_down;
                double* Rw = T + (size_t)(m + l) * ld;
                Rw[rec[l].j] = down ? 1.0 : -1.0;
                Rw[n + l] = 1.0;
                Rw[nn2] = down ? floor(rec[l].v) : -ceil(rec[l].v);
            }
            for (int j = 0; j < n; ++j) T[(size_t)mm2 * ld + j] = c[j];
            memcpy(N, rec[top].basis, sizeof(int) * (size_t)(mm2 - 1));
            N[mm2 - 1] = n + top;
            ++stats[0];
            if (L > stats[3]) stats[3] = L;
            st = mip_crash(T, mm2, nn2, ld, N);
            if (st == REF_OPTIMAL) st = mip_classify_run(T, mm2, nn2, ld, N, maximize, eps, max_iter, &stats[1], &stats[2]);
        }
        /* ---- status and bound */
        int have_open = have_ab;
        double zo = zab;
        for (int k = 0; k <= top; ++k)
            if (!rec[k].second_taken || (stop != REF_OPTIMAL && k == top)) {
                if (!have_open || mip_beats(rec[k].z, zo, maximize, 0.0)) zo = rec[k].z;
                have_open = 1;
            }
        if (stop != REF_OPTIMAL) status = stop;
        else if (found) status = (have_ab && mip_beats(zab, zstar, maximize, gap)) ? REF_ITER_LIMIT : REF_OPTIMAL;
        else status = have_ab ? REF_ITER_LIMIT : REF_INFEASIBLE;
        if (found) {
            *found_out = 1;
            *obj_out = zstar;
            *bound_out = (have_open && mip_beats(zo, zstar, maximize, gap)) ? zo : zstar;
        } else {
            if (have_open) *bound_out = zo;
            for (int j = 0; j < n_orig; ++j) x_out[j] = NAN;
        }
    }
    memcpy(stats_out, stats, sizeof(stats));
    for (int k = 0; k < D; ++k) free(rec[k].basis);
    free(x); free(N); free(T);
    return status;
}
