/*
 * mip_bounded_long_step_ref.c — TEST INFRASTRUCTURE ONLY: the search of mip_bounded_snapshots_ref.c with a choice of
 * the ratio test of its dual loops, the definition of the lp_mip_bounded_solve_ratio_ex family.  One more argument,
 * `dual_ratio`, is appended:
 *
 *   dual_ratio 0 (RATIO_TEXTBOOK): ref_mip_bounded_snapshots itself is called; every output is its own.
 *   dual_ratio 1 (RATIO_LONG_STEP): every dual loop of the search is bref_dual_loop_long_step of
 *     bounded_resolve_long_step_ref.c under Dantzig's dual rule: the dual branch of an install (the root's and a
 *     rebuilt second child's), a first child's loop on the live tableau and a restored second child's.  Everything
 *     else of the search (the checks, the install up to its classification, the primal loop, the records, the
 *     snapshots, the bound changes, pruning, branching, the status and the bound) is restated unchanged.
 *       - stats_out[3] counts the dual loops' flips as well as the primal loops';
 *       - max_iter bounds a node's dual pivots alone in a dual loop (a dual iteration makes at most n flips), and its
 *         pivots plus flips in the primal loop, as before;
 *       - "no candidate left", after flips or without one, is REF_INFEASIBLE for that node: the search backtracks, and
 *         the second child comes from the record or the snapshot as always;
 *       - a level's record, and its snapshot if any, are taken before the child's bound change: the flips a child's
 *         loop makes are never in them.
 *   Any other dual_ratio is REF_BAD_ARG before anything else is looked at; no output is written.
 *
 * The two include chains both end in bounded_resolve_ref.c and bounded_ref.c, which have no include guards.  The
 * search's chain is included first and keeps its names.  The re-solve's chain follows with every name that those two
 * files define sent to an lsr_ twin by the macros below, so it brings a second copy of them (the struct lsr_bref_t has
 * bref_t's members in bref_t's order; the enumerators keep their values) and bref_dual_loop_long_step works on an
 * lsr_bref_t.  The search hands it a view: an lsr_bref_t holding the same m, n, W, eps and the same six pointers as its
 * own bref_t (no loop and no install replaces a pointer, they write through them).
 *
 * diag_out (may be NULL), 8 ints for the tests to show what their inputs reach: [0] second children restored that ended
 * REF_INFEASIBLE; flips made by the dual loop of [1] the root, [2] first children, [3] rebuilt second children, [4]
 * restored second children; [5] nodes whose dual loop ended REF_INFEASIBLE after at least one flip; [6] nodes whose dual
 * loop ended REF_ITER_LIMIT; [7] nodes that ran a dual loop.  Under RATIO_TEXTBOOK only [0] is written, the rest are 0.
 *
 * Built with -ffp-contract=off (simplexmethod_amd/build.py: build_mip_bounded_long_step_ref).  Only tests load it.
 */
#include "mip_bounded_snapshots_ref.c"

#define REF_OPTIMAL lsr_REF_OPTIMAL
#define REF_UNBOUNDED lsr_REF_UNBOUNDED
#define REF_ITER_LIMIT lsr_REF_ITER_LIMIT
#define REF_SINGULAR lsr_REF_SINGULAR
#define REF_INFEASIBLE lsr_REF_INFEASIBLE
#define REF_BAD_ARG lsr_REF_BAD_ARG
#define bref_t lsr_bref_t
#define bref_pivot lsr_bref_pivot
#define bref_loop lsr_bref_loop
#define bref_dual_loop lsr_bref_dual_loop
#define ref_bounded lsr_ref_bounded
#define ref_bounded_resolve lsr_ref_bounded_resolve
#include "bounded_resolve_long_step_ref.c"
#undef REF_OPTIMAL
#undef REF_UNBOUNDED
#undef REF_ITER_LIMIT
#undef REF_SINGULAR
#undef REF_INFEASIBLE
#undef REF_BAD_ARG
#undef bref_t
#undef bref_pivot
#undef bref_loop
#undef bref_dual_loop
#undef ref_bounded
#undef ref_bounded_resolve

typedef struct {
    bref_t* s;
    lsr_bref_t view;   /* the same tableau for bref_dual_loop_long_step */
    int maximize, max_iter;
    int* stats;        /* the search's: [1] dual pivots, [3] flips */
    int* diag;         /* 8, see above */
    double *prow, *lcol;
} mipbl_t;

/* one node's dual loop: stats[1] and stats[3] counted, `kind` (1 root, 2 first child, 3 rebuilt, 4 restored) for diag */
static int mipbl_dual(mipbl_t* q, int kind) {
    int piv = 0, flips = 0;
    const int st = bref_dual_loop_long_step(&q->view, DUAL_DANTZIG, NULL, q->maximize, q->max_iter, &piv, &flips,
                                            q->prow, q->lcol);
    q->stats[1] += piv;
    q->stats[3] += flips;
    q->diag[kind] += flips;
    q->diag[5] += st == REF_INFEASIBLE && flips > 0;
    q->diag[6] += st == REF_ITER_LIMIT;
    ++q->diag[7];
    return st;
}

/* mbref_install with the long-step loop in its dual branch: its set-up, crash and classification are run by
 * mbref_install itself with max_iter 0 (both of its loops return REF_ITER_LIMIT at once then, without a pivot), the
 * classification is restated to see which loop that was */
static int mipbl_install(mipbl_t* q, const double* A, const double* b, const double* c, const double* lo,
                         const double* hi, const int* N, const int* upin, int kind, int* rowpos) {
    bref_t* s = q->s;
    const int m = s->m, n = s->n;
    const double eps = s->eps;
    int none[3] = {0, 0, 0};
    const int st0 = mbref_install(s, A, b, c, lo, hi, N, upin, q->maximize, 0, none, q->prow, q->lcol, rowpos);
    if (st0 != REF_ITER_LIMIT) return st0;   /* REF_INFEASIBLE (hi < lo), REF_SINGULAR, REF_BAD_ARG (no valid start) */
    int violated = 0;
    for (int t = 0; t < m; ++t) {
        const double xb = TT(s, t, n), u = s->U[s->basis[t]];
        if (xb < -eps || (u < INFINITY && u - xb < -eps)) violated = 1;
    }
    if (violated) return mipbl_dual(q, kind);
    int node[3] = {0, 0, 0};
    const int st = bref_loop(s, 1, q->maximize, q->max_iter, &node[1], &node[2], q->prow, q->lcol);
    q->stats[2] += node[1];
    q->stats[3] += node[2];
    return st;
}

int ref_mip_bounded_long_step(const double* A, int m, int n, const double* b, const double* c, const double* lo,
                              const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig,
                              const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes,
                              int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out,
                              int* stats_out, int snapshots, int* diag_out, int dual_ratio) {
    if (dual_ratio != RATIO_TEXTBOOK && dual_ratio != RATIO_LONG_STEP) return REF_BAD_ARG;
    if (dual_ratio == RATIO_TEXTBOOK) {
        int ri = 0;
        const int st = ref_mip_bounded_snapshots(A, m, n, b, c, lo, hi, basis_in, at_upper_in, maximize, n_orig, integer,
                                                 eps, int_tol, gap, max_depth, max_nodes, max_iter, x_out, obj_out,
                                                 bound_out, found_out, stats_out, snapshots, &ri);
        if (diag_out && x_out && obj_out && bound_out && found_out && stats_out) {
            for (int k = 0; k < 8; ++k) diag_out[k] = 0;
            diag_out[0] = ri;
        }
        return st;
    }
    if (snapshots < 0 || snapshots > MIPBS_MAX_SNAPSHOTS) return REF_BAD_ARG;
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

    const int D = max_depth, W = n + 1, nv = n + m, K = snapshots;
    const size_t Tn = (size_t)(m + 1) * W;
    bref_t S;
    bref_t* s = &S;
    s->m = m;
    s->n = n;
    s->W = W;
    s->eps = eps;
    s->T = (double*)mb_alloc(sizeof(double) * Tn);
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
    mipbs_slot* slot = (mipbs_slot*)mb_alloc(sizeof(mipbs_slot) * (size_t)K);
    for (int k = 0; k < K; ++k) {
        slot[k].level = -1;
        slot[k].T = NULL;
    }
    int stats[7] = {0, 0, 0, 0, 0, 0, 0};
    int diag[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < n_orig; ++j) x_out[j] = NAN;
    *obj_out = NAN;
    *bound_out = NAN;
    *found_out = 0;

    mipbl_t Q;
    mipbl_t* q = &Q;
    q->s = s;
    q->view.m = m;
    q->view.n = n;
    q->view.W = W;
    q->view.eps = eps;
    q->view.T = s->T;
    q->view.U = s->U;
    q->view.slotvar = s->slotvar;
    q->view.basis = s->basis;
    q->view.up = s->up;
    q->view.varslot = s->varslot;
    q->maximize = maximize;
    q->max_iter = max_iter;
    q->stats = stats;
    q->diag = diag;
    q->prow = prow;
    q->lcol = lcol;

    /* ---- root */
    memcpy(lov, lo, sizeof(double) * (size_t)n);
    int st = mipbl_install(q, A, b, c, lo, hi, basis_in, at_upper_in, 1, rowpos);
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
                        if (K > 0) {   /* ---- step 4': the state before the bound change into slot L mod K */
                            mipbs_slot* p = &slot[L % K];
                            if (!p->T) {
                                p->T = (double*)mb_alloc(sizeof(double) * Tn);
                                p->U = (double*)mb_alloc(sizeof(double) * (size_t)nv);
                                p->lov = (double*)mb_alloc(sizeof(double) * (size_t)n);
                                p->up = (int*)mb_alloc(sizeof(int) * (size_t)nv);
                                p->basis = (int*)mb_alloc(sizeof(int) * (size_t)m);
                                p->slotvar = (int*)mb_alloc(sizeof(int) * (size_t)n);
                                p->varslot = (int*)mb_alloc(sizeof(int) * (size_t)nv);
                            }
                            p->level = L;
                            memcpy(p->T, s->T, sizeof(double) * Tn);
                            memcpy(p->U, s->U, sizeof(double) * (size_t)nv);
                            memcpy(p->lov, lov, sizeof(double) * (size_t)n);
                            memcpy(p->up, s->up, sizeof(int) * (size_t)nv);
                            memcpy(p->basis, s->basis, sizeof(int) * (size_t)m);
                            memcpy(p->slotvar, s->slotvar, sizeof(int) * (size_t)n);
                            memcpy(p->varslot, s->varslot, sizeof(int) * (size_t)nv);
                        }
                        int t = 0;
                        while (t < m && s->basis[t] != jb) ++t;
                        if (t == m) { stop = REF_BAD_ARG; break; }
                        const double Un = mipbs_change_bound(s, lov, t, jb, v, R->first_down);
                        ++L;
                        ++stats[0];
                        if (L > stats[4]) stats[4] = L;
                        st = Un < 0.0 ? REF_INFEASIBLE : mipbl_dual(q, 2);
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
            L = top + 1;
            ++stats[0];
            if (L > stats[4]) stats[4] = L;
            if (K > 0 && slot[top % K].level == top) {
                /* ---- step 6': the second child from the snapshot of level `top`, the other side */
                mipbs_slot* p = &slot[top % K];
                p->level = -1;
                ++stats[5];
                memcpy(s->T, p->T, sizeof(double) * Tn);
                memcpy(s->U, p->U, sizeof(double) * (size_t)nv);
                memcpy(lov, p->lov, sizeof(double) * (size_t)n);
                memcpy(s->up, p->up, sizeof(int) * (size_t)nv);
                memcpy(s->basis, p->basis, sizeof(int) * (size_t)m);
                memcpy(s->slotvar, p->slotvar, sizeof(int) * (size_t)n);
                memcpy(s->varslot, p->varslot, sizeof(int) * (size_t)nv);
                const int jb = rec[top].j;
                int t = 0;
                while (t < m && s->basis[t] != jb) ++t;
                if (t == m) { stop = REF_BAD_ARG; break; }
                const double Un = mipbs_change_bound(s, lov, t, jb, rec[top].v, !rec[top].first_down);
                st = Un < 0.0 ? REF_INFEASIBLE : mipbl_dual(q, 4);
                diag[0] += st == REF_INFEASIBLE;
                continue;
            }
            /* ---- step 6, the rebuild: the path's bounds, the recorded basis and flags */
            ++stats[6];
            memcpy(lov, lo, sizeof(double) * (size_t)n);
            memcpy(hiv, hi, sizeof(double) * (size_t)n);
            for (int l = 0; l < L; ++l) {
                const int down = rec[l].second_taken ? !rec[l].first_down : rec[l].first_down;
                if (down) hiv[rec[l].j] = floor(rec[l].v);
                else lov[rec[l].j] = ceil(rec[l].v);
            }
            st = mipbl_install(q, A, b, c, lov, hiv, rec[top].basis, rec[top].up, 3, rowpos);
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
    if (diag_out) memcpy(diag_out, diag, sizeof(diag));
    for (int k = 0; k < K; ++k)
        if (slot[k].T) {
            free(slot[k].varslot); free(slot[k].slotvar); free(slot[k].basis); free(slot[k].up);
            free(slot[k].lov); free(slot[k].U); free(slot[k].T);
        }
    free(slot);
    for (int k = 0; k < D; ++k) {
        free(rec[k].up);
        free(rec[k].basis);
    }
    free(rec); free(x); free(hiv); free(lov); free(rowpos); free(lcol); free(prow);
    free(s->varslot); free(s->up); free(s->basis); free(s->slotvar); free(s->U); free(s->T);
    return status;
}
