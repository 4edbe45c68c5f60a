/*
 * mip_bounded_ref.c — TEST INFRASTRUCTURE ONLY: depth-first branch-and-bound OVER VARIABLE BOUNDS for a mixed-integer
 * LP (the lp_mip_bounded_solve family), stated on the arithmetic of bounded_resolve_ref.c (included below: its slot
 * tableau bref_t, bref_pivot, the bounded primal loop bref_loop and the bounded dual loop bref_dual_loop are called,
 * not restated).  Problem: opt c.x, A x = b, lo <= x <= hi as lp_simplex_bounded defines it, x_j integral for every
 * j < n_orig with integer[j] = 1.  A branch changes one bound; the tableau stays (m+1) x (n+1) at every depth.
 *
 *   1. checks: ref_bounded_resolve's (lo_j NaN or infinite, hi_j NaN, basis_in[t] outside [0, n), at_upper_in[j] not
 *      0 or 1, or 1 with hi_j = +inf) and ref_mip's (mask entries other than 0 / 1, a mark at j >= n_orig, int_tol
 *      outside [0, 0.5), gap < 0, max_nodes < 1) with max_depth in [0, 1024]; a marked column whose lo_j, or whose
 *      finite hi_j, is not an integer -> REF_BAD_ARG.  So a non-basic marked column always sits on an integer and the
 *      branching variable is always basic;
 *   2. install (the root and every second child): ref_bounded_resolve steps 2 to 5 on the node's bounds, basis and
 *      flags, kept in mbref_install because that function frees its tableau and the dive needs it: the shift and
 *      complement chains, the crash (skipped for the unit columns in order with zero costs), the classification and
 *      the matching loop.  Some hi_j < lo_j: REF_INFEASIBLE before the crash.  With an all-zero mask the search is one
 *      node and status, x, obj and the three counters are ref_bounded_resolve's bit for bit;
 *   3. a node LP optimum: v_j = xB_t for a basic j, 0 otherwise; w_j = up[j] ? U_j - v_j : v_j; x_j = lo_j == 0 ?
 *      w_j : lo_j + w_j with the node's lo and U; z = sum_{j<n} c_j x_j in index order (no fma).  Pruning, the
 *      integrality test, the branching variable (most fractional marked j, ties to the lowest index) and the side
 *      (down first iff f <= 0.5) are mip_ref.c step 2.  A fractional node at level max_depth is abandoned;
 *   4. branching at level L records (j, v = x_j, z, the first side, the node's basis (m) and flags (n)); the level of
 *      a node is the number of bound changes on its path;
 *   5. first child (dive), O(1) on the live tableau: j is basic at position t with held value w = xB_t, flag f, width
 *      U_j and shift lo_j.
 *        down (hi_j := floor(v)):  U' = floor(v) - lo_j;            if f:  w = w + (U' - U_j);     U_j = U'
 *        up   (lo_j := ceil(v)):   dl = ceil(v) - lo_j; U' = U_j - dl; lo_j = lo_j + dl; if !f: w = w - dl; U_j = U'
 *      (an infinite U_j stays infinite).  U' < 0: the child is REF_INFEASIBLE without a pivot.  Else the basis is
 *      still dual feasible and bref_dual_loop runs as it is.  (j not basic cannot happen under check 1; the search
 *      would stop REF_BAD_ARG);
 *   6. second child (rebuild) of level `top`: bounds = the root's lo / hi overlaid in level order with the records
 *      0 .. top (down: hi_j = floor(v), up: lo_j = ceil(v); the top level on its other side), the basis and flags
 *      recorded at `top`, then the install of step 2;
 *   7. a node LP solve is counted before it starts: with max_nodes solved the search stops (REF_ITER_LIMIT).  A node
 *      that ends REF_INFEASIBLE backtracks; one that ends anything but REF_OPTIMAL / REF_INFEASIBLE stops the search
 *      with that status (max_iter bounds each node's pivots plus flips; a rebuild with no valid start: REF_BAD_ARG);
 *   8. status, found, obj and bound: mip_ref.c step 7, unchanged.
 *
 * stats_out[5]: nodes solved (the root included), dual pivots, primal pivots, bound flips, deepest level solved.  Crash
 * pivots are not counted.  Built with -ffp-contract=off (simplexmethod_amd/build.py: build_mip_bounded_ref).  Only
 * tests load it.
 */
#include "bounded_resolve_ref.c"

#define MIPB_MAX_DEPTH 1024

static void* mb_alloc(size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p) abort();
    return p;
}

/* step 2: ref_bounded_resolve steps 2 to 5 on s (T, U, slotvar, basis, up, varslot allocated) */
static int mbref_install(bref_t* s, const double* A, const double* b, const double* c, const double* lo,
                         const double* hi, const int* N, const int* upin, int maximize, int max_iter, int* it,
                         double* prow, double* lcol, int* rowpos) {
    const int m = s->m, n = s->n, W = s->W, nv = n + m;
    const double eps = s->eps;
    for (int j = 0; j < n; ++j)
        if (hi[j] < lo[j]) return REF_INFEASIBLE;
    for (int j = 0; j < n; ++j) s->U[j] = hi[j] - lo[j], s->up[j] = upin[j];
    for (int k = n; k < nv; ++k) s->U[k] = INFINITY, s->up[k] = 0;
    for (int j = 0; j < n; ++j) s->slotvar[j] = j, s->varslot[j] = j;
    for (int t = 0; t < m; ++t) s->basis[t] = n + t, s->varslot[n + t] = -1;
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
    }
    for (int j = 0; j < n; ++j) TT(s, m, j) = s->up[j] ? -c[j] : c[j];
    TT(s, m, n) = 0.0;

    int identity = 1;
    for (int t = 0; t < m && identity; ++t)
        for (int i = 0; i < m; ++i)
            if (TT(s, i, N[t]) != ((i == t) ? 1.0 : 0.0)) {
                identity = 0;
                break;
            }
    for (int t = 0; t < m && identity; ++t)
        if (TT(s, m, N[t]) != 0.0) identity = 0;
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
            int p = -1;
            double big = -1.0;
            if (s->slotvar[q] == q)
                for (int i = 0; i < m; ++i) {
                    if (s->basis[i] < n) continue;
                    const double a = fabs(TT(s, i, q));
                    if (a > big) {
                        big = a;
                        p = i;
                    }
                }
            if (!(big > 0.0)) return REF_SINGULAR;
            if (big < minp) minp = big;
            if (big > maxp) maxp = big;
            bref_pivot(s, p, q, prow, lcol);
            rowpos[t] = p;
        }
        if (minp <= DBL_EPSILON * (double)m * maxp) return REF_SINGULAR;
        double* T2 = (double*)mb_alloc(sizeof(double) * (size_t)(m + 1) * W);
        for (int t = 0; t < m; ++t) memcpy(T2 + (size_t)t * W, s->T + (size_t)rowpos[t] * W, sizeof(double) * (size_t)W);
        memcpy(T2 + (size_t)m * W, s->T + (size_t)m * W, sizeof(double) * (size_t)W);
        memcpy(s->T, T2, sizeof(double) * (size_t)(m + 1) * W);
        free(T2);
        for (int t = 0; t < m; ++t) s->basis[t] = N[t];
    }

    int violated = 0, dual_infeasible = 0;
    for (int t = 0; t < m; ++t) {
        const double xb = TT(s, t, n), u = s->U[s->basis[t]];
        if (xb < -eps || (u < INFINITY && u - xb < -eps)) violated = 1;
    }
    for (int sl = 0; sl < n; ++sl) {
        const double dj = TT(s, m, sl);
        if (s->slotvar[sl] < n && (maximize ? (dj > eps) : (dj < -eps))) dual_infeasible = 1;
    }
    int node[3] = {0, 0, 0};
    int st = REF_BAD_ARG;
    if (!violated)
        st = bref_loop(s, 1, maximize, max_iter, &node[1], &node[2], prow, lcol);
    else if (!dual_infeasible)
        st = bref_dual_loop(s, maximize, max_iter, &node[0], prow, lcol);
    for (int k = 0; k < 3; ++k) it[k] += node[k];
    return st;
}

typedef struct {
    int j, first_down, second_taken;
    double v, z;
    int* basis; /* m */
    int* up;    /* n */
} mipb_record;

static int mipb_beats(double z, double zs, int maximize, double gap) {
    return maximize ? (z > zs + gap) : (z < zs - gap);
}

int ref_mip_bounded(const double* A, int m, int n, const double* b, const double* c, const double* lo,
                    const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig,
                    const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes,
                    int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out, int* stats_out) {
    if (m <= 0 || n < m || !A || !b || !c || !lo || !hi || !basis_in || !at_upper_in || !integer) return REF_BAD_ARG;
    if (!x_out || !obj_out || !bound_out || !found_out || !stats_out) return REF_BAD_ARG;
    if (n_orig <= 0 || n_orig > n) return REF_BAD_ARG;
    if (max_depth < 0 || max_depth > MIPB_MAX_DEPTH || max_nodes < 1) return REF_BAD_ARG;
    if (!(int_tol >= 0.0 && int_tol < 0.5) || !(gap >= 0.0)) return REF_BAD_ARG;
    for (int j = 0; j < n; ++j) {
        if (!isfinite(lo[j]) || isnan(hi[j])) return REF_BAD_ARG;
        if (at_upper_in[j] != 0 && at_upper_in[j] != 1) return REF_BAD_ARG;
        if (at_upper_in[j] && hi[j] == INFINITY) return REF_BAD_ARG;
        if ((integer[j] != 0 && integer[j] != 1) || (integer[j] && j >= n_orig)) return REF_BAD_ARG;
        if (integer[j] && (lo[j] != floor(lo[j]) || (isfinite(hi[j]) && hi[j] != floor(hi[j])))) return REF_BAD_ARG;
    }
    for (int t = 0; t < m; ++t)
        if (basis_in[t] < 0 || basis_in[t] >= n) return REF_BAD_ARG;

    const int D = max_depth, W = n + 1, nv = n + m;
    bref_t S;
    bref_t* s = &S;
    s->m = m;
    s->n = n;
    s->W = W;
    s->eps = eps;
    s->T = (double*)mb_alloc(sizeof(double) * (size_t)(m + 1) * W);
    s->U = (double*)mb_alloc(sizeof(double) * (size_t)nv);
    s->slotvar = (int*)mb_alloc(sizeof(int) * (size_t)n);
    s->basis = (int*)mb_alloc(sizeof(int) * (size_t)m);
    s->up = (int*)mb_alloc(sizeof(int) * (size_t)nv);
    s->varslot = (int*)mb_alloc(sizeof(int) * (size_t)nv);
    double* prow = (double*)mb_alloc(sizeof(double) * (size_t)W);
    double* lcol = (double*)mb_alloc(sizeof(double) * (size_t)(m + 1));
    int* rowpos = (int*)mb_alloc(sizeof(int) * (size_t)m);
    double* lov = (double*)mb_alloc(sizeof(double) * (size_t)n);   /* the node's lo */
    double* hiv = (double*)mb_alloc(sizeof(double) * (size_t)n);   /* a rebuild's hi */
    double* x = (double*)mb_alloc(sizeof(double) * (size_t)n);
    mipb_record* rec = (mipb_record*)mb_alloc(sizeof(mipb_record) * (size_t)D);
    for (int k = 0; k < D; ++k) {
        rec[k].basis = (int*)mb_alloc(sizeof(int) * (size_t)m);
        rec[k].up = (int*)mb_alloc(sizeof(int) * (size_t)n);
    }
    int stats[5] = {0, 0, 0, 0, 0};
    for (int j = 0; j < n_orig; ++j) x_out[j] = NAN;
    *obj_out = NAN;
    *bound_out = NAN;
    *found_out = 0;

    /* ---- root */
    memcpy(lov, lo, sizeof(double) * (size_t)n);
    int st = mbref_install(s, A, b, c, lo, hi, basis_in, at_upper_in, maximize, max_iter, &stats[1], prow, lcol, rowpos);
    stats[0] = 1;

    int status = st;
    if (st != REF_OPTIMAL) {
        if (st == REF_UNBOUNDED || st == REF_ITER_LIMIT) *bound_out = maximize ? INFINITY : -INFINITY;
    } else {
        int L = 0, top = -1, found = 0, stop = REF_OPTIMAL, have_ab = 0;
        double zstar = 0.0, zab = 0.0;
        for (;;) {
            int backtrack = 1;
            if (st == REF_OPTIMAL) {
                for (int j = 0; j < n; ++j) x[j] = 0.0;
                for (int t = 0; t < m; ++t)
                    if (s->basis[t] < n) x[s->basis[t]] = TT(s, t, n);
                for (int j = 0; j < n; ++j) {
                    const double w = s->up[j] ? s->U[j] - x[j] : x[j];
                    x[j] = lov[j] == 0.0 ? w : lov[j] + w;
                }
                double z = 0.0;
                for (int j = 0; j < n; ++j) z += c[j] * x[j];
                if (!found || mipb_beats(z, zstar, maximize, gap)) {
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
                        if (!have_ab || mipb_beats(z, zab, maximize, 0.0)) zab = z;
                        have_ab = 1;
                    } else {
                        /* ---- branch: record level L, then the first child on the live tableau */
                        mipb_record* R = &rec[L];
                        const double v = x[jb];
                        R->j = jb;
                        R->v = v;
                        R->z = z;
                        R->first_down = (v - floor(v)) <= 0.5;
                        R->second_taken = 0;
                        memcpy(R->basis, s->basis, sizeof(int) * (size_t)m);
                        memcpy(R->up, s->up, sizeof(int) * (size_t)n);
                        top = L;
                        if (stats[0] >= max_nodes) { stop = REF_ITER_LIMIT; break; }
                        int t = 0;
                        while (t < m && s->basis[t] != jb) ++t;
                        if (t == m) { stop = REF_BAD_ARG; break; }
                        const int f = s->up[jb];
                        const double Uj = s->U[jb];
                        double Un;
                        if (R->first_down) {
                            Un = floor(v) - lov[jb];
                            if (f) TT(s, t, n) = TT(s, t, n) + (Un - Uj);
                        } else {
                            const double dl = ceil(v) - lov[jb];
                            Un = Uj - dl;
                            lov[jb] = lov[jb] + dl;
                            if (!f) TT(s, t, n) = TT(s, t, n) - dl;
                        }
                        s->U[jb] = Un;
                        ++L;
                        ++stats[0];
                        if (L > stats[4]) stats[4] = L;
                        if (Un < 0.0) {
                            st = REF_INFEASIBLE;
                        } else {
                            int itd = 0;
                            st = bref_dual_loop(s, maximize, max_iter, &itd, prow, lcol);
                            stats[1] += itd;
                        }
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
            /* ---- the second child of record `top`: the path's bounds, the recorded basis and flags */
            L = top + 1;
            memcpy(lov, lo, sizeof(double) * (size_t)n);
            memcpy(hiv, hi, sizeof(double) * (size_t)n);
            for (int l = 0; l < L; ++l) {
                const int down = rec[l].second_taken ? !rec[l].first_down : rec[l].first_down;
                if (down) hiv[rec[l].j] = floor(rec[l].v);
                else lov[rec[l].j] = ceil(rec[l].v);
            }
            ++stats[0];
            if (L > stats[4]) stats[4] = L;
            st = mbref_install(s, A, b, c, lov, hiv, rec[top].basis, rec[top].up, maximize, max_iter, &stats[1], prow,
                               lcol, rowpos);
        }
        /* ---- status and bound (mip_ref.c step 7) */
        int have_open = have_ab;
        double zo = zab;
        for (int k = 0; k <= top; ++k)
            if (!rec[k].second_taken || (stop != REF_OPTIMAL && k == top)) {
                if (!have_open || mipb_beats(rec[k].z, zo, maximize, 0.0)) zo = rec[k].z;
                have_open = 1;
            }
        if (stop != REF_OPTIMAL) status = stop;
        else if (found) status = (have_ab && mipb_beats(zab, zstar, maximize, gap)) ? REF_ITER_LIMIT : REF_OPTIMAL;
        else status = have_ab ? REF_ITER_LIMIT : REF_INFEASIBLE;
        if (found) {
            *found_out = 1;
            *obj_out = zstar;
            *bound_out = (have_open && mipb_beats(zo, zstar, maximize, gap)) ? zo : zstar;
        } else {
            if (have_open) *bound_out = zo;
            for (int j = 0; j < n_orig; ++j) x_out[j] = NAN;
        }
    }
    memcpy(stats_out, stats, sizeof(stats));
    for (int k = 0; k < D; ++k) {
        free(rec[k].up);
        free(rec[k].basis);
    }
    free(rec); free(x); free(hiv); free(lov); free(rowpos); free(lcol); free(prow);
    free(s->varslot); free(s->up); free(s->basis); free(s->slotvar); free(s->U); free(s->T);
    return status;
}
