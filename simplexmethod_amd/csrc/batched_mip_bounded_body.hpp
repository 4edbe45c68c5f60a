// batched_mip_bounded_body.hpp — the text of k_batched_mip_bounded<NT> (batched_mip_bounded.hip), included INSIDE the
// kernel: `d` is its BatchedMipBoundedDev, NT its block size.  Not a standalone header.
//
// Under the macro LP_BOUNDED_DUAL_LONG_STEP (k_batched_mip_bounded_long; tests/ref/mip_bounded_long_step_ref.c states the
// search) batched_bounded_dual_loop.hpp's loop is its bound-flipping form and takes a second counter: the install's dual
// branch and the first child's loop add their flips to st_flips.  The records are written before a child's bound
// change, so a child's flips never reach them.  Without the macro the code is what it was.
    constexpr bool BLAND = false;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    char* base = reinterpret_cast<char*>(smem);
    const int m = d.m, n = d.n, W = n + 1, D = d.max_depth;
    const BoundedCarve K = bounded_carve(m, n);
    const MipBoundedCarve R = mip_bounded_carve(m, n, D);
    const int pitch = K.pitch, FW = R.fw;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = reinterpret_cast<double*>(base + K.T);
    double* prow = reinterpret_cast<double*>(base + K.prow);
    double* lcol = reinterpret_cast<double*>(base + K.lcol);
    double* U = reinterpret_cast<double*>(base + K.U);
    double* lov = reinterpret_cast<double*>(base + K.lov);
    int* slotvar = reinterpret_cast<int*>(base + K.slotvar);
    int* basis = reinterpret_cast<int*>(base + K.basis);
    int* up = reinterpret_cast<int*>(base + K.up);
    double* recv = reinterpret_cast<double*>(base + R.recv);
    double* recz = reinterpret_cast<double*>(base + R.recz);
    int* recj = reinterpret_cast<int*>(base + R.recj);
    int* recf = reinterpret_cast<int*>(base + R.recf);
    int* pbasis = reinterpret_cast<int*>(base + R.pbasis);
    unsigned* pflags = reinterpret_cast<unsigned*>(base + R.pflags);
    int* mipw = reinterpret_cast<int*>(base + R.mipw);
    int* pub = pubs->v;   // [0] entering slot / crash row, [1] leaving position, [2] action / verdict, [3] block_any

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* lo = d.lo + (size_t)lp * n;
    const double* hi = d.hi + (size_t)lp * n;
    const int no = d.n_orig;
    const double eps = d.eps, gap = d.gap;
    const bool maximize = d.maximize != 0;
    double* xo = d.x + (size_t)lp * no;

    if (d.root_status && d.root_status[lp] != LP_OPTIMAL) {   // (uniform over the workgroup: no barrier follows)
        for (int j = tid; j < no; j += NT) xo[j] = NAN;
        if (tid < 5) d.stats[(size_t)lp * 5 + tid] = 0;
        if (tid == 0) {
            d.obj[lp] = NAN;
            d.bound[lp] = NAN;
            d.found[lp] = 0;
            d.status[lp] = d.root_status[lp];
        }
        return;
    }
    for (int j = tid; j < no; j += NT) xo[j] = NAN;

    constexpr int ANY_WORD = 3;   // block_any's word of pub
#include "batched_block_any.hpp"

    // ---- pivot(r, se); the bounded primal loop; the bounded dual loop
#include "batched_lds_loop.hpp"
#include "batched_bounded_loop.hpp"
#include "batched_bounded_dual_loop.hpp"
    (void)simplex;   // (batched_lds_loop.hpp's unbounded loop: only its pivot is used here)

    int nodes = 1, st_dual = 0, st_primal = 0, st_flips = 0, deepest = 0;

    // ---- install: k_batched_bounded_resolve from its load to its loop, on lov (the node's lo), U (holding the node's
    // hi on entry) and up, from the basis N (HBM for the root, a level's record for a rebuild)
    auto install = [&](const int* N) __attribute__((always_inline)) -> int {
        int bad = 0;
        for (int s = tid; s < n; s += NT) {
            const double u = U[s] - lov[s];
            slotvar[s] = s;
            U[s] = u;
            T[(size_t)m * pitch + s] = up[s] ? -c[s] : c[s];
            if (u < 0.0) bad = 1;
        }
        if (tid == 0) T[(size_t)m * pitch + n] = 0.0;
        for (int t = tid; t < m; t += NT) basis[t] = n + t;
        for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
            const int s = e / m, i = e - s * m;
            const double a = A[e];
            T[(size_t)i * pitch + s] = up[s] ? -a : a;
        }
        if (block_any(bad)) return LP_INFEASIBLE;   // some hi < lo
        // b' (one chain per row): the shift over lo_j != 0, then the complements over the flagged columns
        for (int i = tid; i < m; i += NT) {
            const double* row = T + (size_t)i * pitch;
            double acc = b[i];
            for (int j = 0; j < n; ++j) {
                const double l = lov[j];
                if (l != 0.0) acc = fma(up[j] ? row[j] : -row[j], l, acc);   // (-A_ij: a flagged slot holds it)
            }
            for (int j = 0; j < n; ++j)
                if (up[j]) acc = fma(row[j], U[j], acc);
            T[(size_t)i * pitch + n] = acc;
        }
        int not_identity = 0;
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m;
            if (T[(size_t)i * pitch + N[t]] != ((i == t) ? 1.0 : 0.0)) not_identity = 1;
        }
        for (int t = tid; t < m; t += NT)
            if (T[(size_t)m * pitch + N[t]] != 0.0) not_identity = 1;
        const bool identity = !block_any(not_identity);
        int status = LP_OPTIMAL;
#include "batched_resolve_crash.hpp"
        if (status != LP_OPTIMAL) return status;
        // classification: two block reductions over the crashed tableau
        int pinf = 0, dinf = 0;
        for (int t = tid; t < m; t += NT) {
            const double xb = T[(size_t)t * pitch + n], u = U[basis[t]];
            if (xb < -eps || (u < INFINITY && u - xb < -eps)) pinf = 1;
        }
        const double* drow = T + (size_t)m * pitch;
        for (int s = tid; s < n; s += NT)
            if (slotvar[s] < n && (maximize ? (drow[s] > eps) : (drow[s] < -eps))) dinf = 1;
        const bool violated = block_any(pinf);
        const bool dual_feasible = !block_any(dinf);
        int itd = 0, itp = 0, itf = 0;
        if (!violated)
            status = bounded_simplex(true, maximize, itp, itf);   // artificial slots barred
        else if (dual_feasible)
#ifdef LP_BOUNDED_DUAL_LONG_STEP
            status = bounded_dual(itd, itf);
#else
            status = bounded_dual(itd);
#endif
        else
            status = LP_BAD_ARG;
        st_dual += itd;
        st_primal += itp;
        st_flips += itf;
        __syncthreads();
        return status;
    };

    // ---- root: the given bounds and flags
    for (int s = tid; s < n; s += NT) {
        lov[s] = lo[s];
        U[s] = hi[s];
        up[s] = d.at_upper_in[(size_t)lp * n + s];
    }
    __syncthreads();
    // one call site for the install: the root, then each second child as the turn before prepared it
    const int* N = d.basis_in + (size_t)lp * m;
    int st = LP_OPTIMAL, status = LP_OPTIMAL, found = 0;
    double zstar = 0.0, bound = NAN;
    bool root_failed = false;
    {
        int L = 0, top = -1, stop = LP_OPTIMAL;
        bool have_ab = false;
        double zab = 0.0;
        for (;;) {
            if (N) {
                st = install(N);
                N = nullptr;
                if (nodes == 1 && st != LP_OPTIMAL) {
                    root_failed = true;
                    break;
                }
            }
            bool backtrack = true;
            if (st == LP_OPTIMAL) {
                // ---- evaluate: x of the node (true values) in prow, z by thread 0 in index order, the branching
                // variable by wave 0
                for (int j = tid; j < n; j += NT) prow[j] = 0.0;
                __syncthreads();
                for (int t = tid; t < m; t += NT)
                    if (basis[t] < n) prow[basis[t]] = T[(size_t)t * pitch + n];
                __syncthreads();
                for (int j = tid; j < n; j += NT) {
                    const double v = prow[j];
                    const double w = up[j] ? U[j] - v : v;
                    prow[j] = lov[j] == 0.0 ? w : lov[j] + w;
                }
                __syncthreads();
                double z = 0.0;
                if (wave == 0) {
                    double bd = 0.0;
                    int bj = INT_MAX;
                    for (int j = lane; j < no; j += 64) {
                        if (!d.integer[j]) continue;
                        const double v = prow[j];
                        const double f = v - floor(v);
                        const double dist = f < 1.0 - f ? f : 1.0 - f;
                        if (dist > d.int_tol && dist > bd) {   // j ascending per lane: strict > keeps the lowest
                            bd = dist;
                            bj = j;
                        }
                    }
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const double ob = __shfl_xor(bd, off, 64);
                        const int oj = __shfl_xor(bj, off, 64);
                        if (ob > bd || (ob == bd && oj < bj)) {
                            bd = ob;
                            bj = oj;
                        }
                    }
                    if (lane == 0) {
                        for (int j = 0; j < n; ++j) z += c[j] * prow[j];
                        mipw[0] = bj == INT_MAX ? -1 : bj;
                        mipw[1] = -1;
                        lcol[0] = z;
                    }
                }
                __syncthreads();
                z = lcol[0];
                const int jb = mipw[0];
                if (!found || mipb_beats(z, zstar, maximize, gap)) {
                    if (jb < 0) {   // integral: the new incumbent
                        found = 1;
                        zstar = z;
                        for (int j = tid; j < no; j += NT) xo[j] = prow[j];
                    } else if (L == D) {   // fractional at the depth limit: abandoned
                        if (!have_ab || mipb_beats(z, zab, maximize, 0.0)) zab = z;
                        have_ab = true;
                    } else {
                        // ---- branch: the record of level L, then the first child on the live tableau
                        const double v = prow[jb];
                        const bool down = (v - floor(v)) <= 0.5;
                        for (int t = tid; t < m; t += NT) {
                            pbasis[(size_t)L * m + t] = basis[t];
                            if (basis[t] == jb) mipw[1] = t;
                        }
                        for (int j0 = wave * 64; j0 < n; j0 += NT) {   // one ballot packs 64 flags: two words
                            const int j = j0 + lane;
                            const unsigned long long bits = __ballot(j < n && up[j] != 0);
                            const int w = j0 >> 5;
                            if (lane == 0) pflags[(size_t)L * FW + w] = (unsigned)bits;
                            if (lane == 0 && w + 1 < FW) pflags[(size_t)L * FW + w + 1] = (unsigned)(bits >> 32);
                        }
                        if (tid == 0) {
                            recj[L] = jb;
                            recf[L] = down ? 1 : 0;
                            recv[L] = v;
                            recz[L] = z;
                        }
                        top = L;
                        if (nodes >= d.max_nodes) {
                            stop = LP_ITER_LIMIT;
                            break;
                        }
                        __syncthreads();
                        const int t = mipw[1];
                        if (t < 0) {   // (the branching variable is basic: the entry refuses fractional bounds)
                            stop = LP_BAD_ARG;
                            break;
                        }
                        // the new bound: U_j, lo_j and the held value of position t (mip_bounded_ref.c step 5)
                        const int f = up[jb];
                        const double Uj = U[jb], lj = lov[jb];
                        double Un;
                        if (down) {
                            Un = floor(v) - lj;
                        } else {
                            Un = Uj - (ceil(v) - lj);
                        }
                        __syncthreads();   // (every thread has read U, lov and up of jb)
                        if (tid == 0) {
                            double* xb = T + (size_t)t * pitch + n;
                            if (down) {
                                if (f) *xb = *xb + (Un - Uj);
                            } else {
                                const double dl = ceil(v) - lj;
                                lov[jb] = lj + dl;
                                if (!f) *xb = *xb - dl;
                            }
                            U[jb] = Un;
                        }
                        __syncthreads();
                        ++L;
                        ++nodes;
                        if (L > deepest) deepest = L;
                        if (Un < 0.0) {
                            st = LP_INFEASIBLE;
                        } else {
                            int it = 0;
#ifdef LP_BOUNDED_DUAL_LONG_STEP
                            int fl = 0;
                            st = bounded_dual(it, fl);
                            st_flips += fl;
#else
                            st = bounded_dual(it);
#endif
                            st_dual += it;
                            __syncthreads();
                        }
                        backtrack = false;
                    }
                }
            } else if (st != LP_INFEASIBLE) {
                stop = st;
                break;
            }
            if (!backtrack) continue;
            // ---- backtrack to the deepest level whose second child is pending
            __syncthreads();   // (recf as thread 0 last wrote it)
            while (top >= 0 && (recf[top] & 2)) --top;
            if (top < 0) break;
            __syncthreads();
            if (tid == 0) recf[top] |= 2;
            if (nodes >= d.max_nodes) {
                stop = LP_ITER_LIMIT;
                break;
            }
            // ---- the second child of level `top`: the root's bounds overlaid with the path's records in level
            // order (the top level on its other side), the recorded basis and flags
            L = top + 1;
            for (int s = tid; s < n; s += NT) {
                lov[s] = lo[s];
                U[s] = hi[s];
                up[s] = (pflags[(size_t)top * FW + (s >> 5)] >> (s & 31)) & 1u;
            }
            __syncthreads();
            if (tid == 0)
                for (int l = 0; l < L; ++l) {
                    const int f = recf[l];
                    const bool dn = (f & 2) ? !(f & 1) : (f & 1);
                    if (dn) U[recj[l]] = floor(recv[l]);
                    else lov[recj[l]] = ceil(recv[l]);
                }
            __syncthreads();
            ++nodes;
            if (L > deepest) deepest = L;
            N = pbasis + (size_t)top * m;
        }
        __syncthreads();   // (the records tid 0 wrote last)
        // ---- status and bound (mip_ref.c step 7); a root that is not optimal gives its status
        bool have_open = have_ab;
        double zo = zab;
        for (int k = 0; k <= top; ++k)
            if (!(recf[k] & 2) || (stop != LP_OPTIMAL && k == top)) {
                if (!have_open || mipb_beats(recz[k], zo, maximize, 0.0)) zo = recz[k];
                have_open = true;
            }
        if (root_failed) status = st;
        else if (stop != LP_OPTIMAL) status = stop;
        else if (found) status = (have_ab && mipb_beats(zab, zstar, maximize, gap)) ? LP_ITER_LIMIT : LP_OPTIMAL;
        else status = have_ab ? LP_ITER_LIMIT : LP_INFEASIBLE;
        if (root_failed) {
            if (st == LP_UNBOUNDED || st == LP_ITER_LIMIT) bound = maximize ? INFINITY : -INFINITY;
        } else if (found) {
            bound = (have_open && mipb_beats(zo, zstar, maximize, gap)) ? zo : zstar;
        } else if (have_open) {
            bound = zo;
        }
    }
    if (tid == 0) {
        d.status[lp] = status;
        d.found[lp] = found;
        d.obj[lp] = found ? zstar : NAN;
        d.bound[lp] = bound;
        int* so = d.stats + (size_t)lp * 5;
        so[0] = nodes;
        so[1] = st_dual;
        so[2] = st_primal;
        so[3] = st_flips;
        so[4] = deepest;
    }
