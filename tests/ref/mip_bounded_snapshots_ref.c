/*
 * mip_bounded_snapshots_ref.c — TEST INFRASTRUCTURE ONLY: the search of mip_bounded_ref.c (included below: its
 * install mbref_install, its record, mipb_beats and, through it, bref_dual_loop are called, not restated) with up to
 * K tableau snapshots, the definition of lp_mip_bounded_solve_large_ex.  Only the search loop is restated, with one
 * more argument `snapshots` = K >= 0 (outside [0, 1024]: REF_BAD_ARG before anything else).  Steps 1 to 3, 5, 7 and 8
 * of mip_bounded_ref.c stand; two steps change:
 *
 *   4'. when level L branches and its dive is going to run (after the max_nodes check of step 4), and K > 0: the
 *       node's state as it is BEFORE the first child's bound change (the tableau, U, the node's lo, the flags and the
 *       basis, with the slot maps that go with them) is stored in slot L mod K.  The slot now belongs to level L;
 *       whatever it held is gone;
 *   6'. the second child of record `top`: if slot top mod K still belongs to level top, the state is restored and
 *       step 5 is applied with the OTHER side, from the recorded j and v (the column is basic at the position where
 *       the snapshot's basis holds it; U' < 0: REF_INFEASIBLE without a pivot; else bref_dual_loop as it is; no
 *       crash, no classification).  Otherwise step 6 unchanged, the rebuild.  The node is counted, and the budget
 *       checked, exactly as in step 6.
 *
 * A new record at level L can only appear after the old record of level L has had its second child and its whole
 * subtree, so the tag of a slot is only ever overwritten by level L + K, L + 2K, ...: with K >= max_depth every
 * second child is restored, with a smaller K the ring keeps the K deepest pending levels.  K = 0 is the search of
 * mip_bounded_ref.c bit for bit.
 *
 * stats_out[7]: the five counters of mip_bounded_ref.c, then the second children restored, then the second children
 * rebuilt.  restored_infeasible_out (may be NULL): how many restored children ended REF_INFEASIBLE (the tests show
 * with it that their inputs reach that outcome).  Built with -ffp-contract=off (simplexmethod_amd/build.py).  Only
 * tests load it.
 */
#include "mip_bounded_ref.c"

#define MIPBS_MAX_SNAPSHOTS 1024

typedef struct {
    int level; /* the level the slot belongs to, -1: none */
    double *T, *U, *lov;
    int *up, *basis, *slotvar, *varslot;
} mipbs_slot;

/* step 5 on the live tableau: the bound change of column jb (basic at position t) to the side `down`, from the
 * branching value v; returns U' */
static double mipbs_change_bound(bref_t* s, double* lov, int t, int jb, double v, int down) {
    const int n = s->n;
    const int f = s->up[jb];
    const double Uj = s->U[jb];
    double Un;
    if (down) {
        Un = floor(v) - lov[jb];
        if (f) TT(s, t, n) = TT(s, t, n) + (Un - Uj);
    } else {
        const double dl = ceil(v) - lov[jb];
        Un = Uj - dl;
        lov[jb] = lov[jb] + dl;
        if (!f) TT(s, t, n) = TT(s, t, n) - dl;
    }
    s->U[jb] = Un;
    return Un;
}

int ref_mip_bounded_snapshots(const double* A, int m, int n, const double* b, const double* c, const double* lo,
                              const double* hi, const int* basis_in, const int* at_upper_in, int maximize, int n_orig,
                              const int* integer, double eps, double int_tol, double gap, int max_depth, int max_nodes,
                              int max_iter, double* x_out, double* obj_out, double* bound_out, int* found_out,
                              int* stats_out, int snapshots, int* restored_infeasible_out) {
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
    /* the ring: a slot is allocated when it is first written */
    mipbs_slot* slot = (mipbs_slot*)mb_alloc(sizeof(mipbs_slot) * (size_t)K);
    for (int k = 0; k < K; ++k) {
        slot[k].level = -1;
        slot[k].T = NULL;
    }
    int stats[7] = {0, 0, 0, 0, 0, 0, 0};
    int restored_infeasible = 0;
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
                        if (K > 0) {   /* ---- step 4': the state before the bound change into slot L mod K */
                            mipbs_slot* q = &slot[L % K];
                            if (!q->T) {
                                q->T = (double*)mb_alloc(sizeof(double) * Tn);
                                q->U = (double*)mb_alloc(sizeof(double) * (size_t)nv);
                                q->lov = (double*)mb_alloc(sizeof(double) * (size_t)n);
                                q->up = (int*)mb_alloc(sizeof(int) * (size_t)nv);
                                q->basis = (int*)mb_alloc(sizeof(int) * (size_t)m);
                                q->slotvar = (int*)mb_alloc(sizeof(int) * (size_t)n);
                                q->varslot = (int*)mb_alloc(sizeof(int) * (size_t)nv);
                            }
                            q->level = L;
                            memcpy(q->T, s->T, sizeof(double) * Tn);
                            memcpy(q->U, s->U, sizeof(double) * (size_t)nv);
                            memcpy(q->lov, lov, sizeof(double) * (size_t)n);
                            memcpy(q->up, s->up, sizeof(int) * (size_t)nv);
                            memcpy(q->basis, s->basis, sizeof(int) * (size_t)m);
                            memcpy(q->slotvar, s->slotvar, sizeof(int) * (size_t)n);
                            memcpy(q->varslot, s->varslot, sizeof(int) * (size_t)nv);
                        }
                        int t = 0;
                        while (t < m && s->basis[t] != jb) ++t;
                        if (t == m) { stop = REF_BAD_ARG; break; }
                        const double Un = mipbs_change_bound(s, lov, t, jb, v, R->first_down);
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
            L = top + 1;
            ++stats[0];
            if (L > stats[4]) stats[4] = L;
            if (K > 0 && slot[top % K].level == top) {
                /* ---- step 6': the second child from the snapshot of level `top`, the other side */
                mipbs_slot* q = &slot[top % K];
                q->level = -1;
                ++stats[5];
                memcpy(s->T, q->T, sizeof(double) * Tn);
                memcpy(s->U, q->U, sizeof(double) * (size_t)nv);
                memcpy(lov, q->lov, sizeof(double) * (size_t)n);
                memcpy(s->up, q->up, sizeof(int) * (size_t)nv);
                memcpy(s->basis, q->basis, sizeof(int) * (size_t)m);
                memcpy(s->slotvar, q->slotvar, sizeof(int) * (size_t)n);
                memcpy(s->varslot, q->varslot, sizeof(int) * (size_t)nv);
                const int jb = rec[top].j;
                int t = 0;
                while (t < m && s->basis[t] != jb) ++t;
                if (t == m) { stop = REF_BAD_ARG; break; }
                const double Un = mipbs_change_bound(s, lov, t, jb, rec[top].v, !rec[top].first_down);
                if (Un < 0.0) {
                    st = REF_INFEASIBLE;
                } else {
                    int itd = 0;
                    st = bref_dual_loop(s, maximize, max_iter, &itd, prow, lcol);
                    stats[1] += itd;
                }
                restored_infeasible += st == REF_INFEASIBLE;
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
    if (restored_infeasible_out) *restored_infeasible_out = restored_infeasible;
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
