// batched_mip.hip — depth-first BRANCH-AND-BOUND for many integer LPs of one shape, ONE PROBLEM PER WORKGROUP.
//
// Each workgroup runs tests/ref/mip_ref.c's search with the tableau and the whole search state in LDS: no global
// scratch, no host round trip per node.  The root is batched_resolve.hip's re-solve (the same crash, classification,
// primal and dual loops, included); a node that branches records (j, v, z, side, basis) for its level, then
//   - first child (dive): one row and one slack appended in tableau form to the node's final tableau (row t of x_j
//     with the sign fixed, rhs floor(v) - v or v - ceil(v)), O(n + L) writes; the basis stays dual feasible and the
//     dual loop (batched_dual_loop.hpp) runs;
//   - second child (rebuild): T = [A | 0 | b] plus the branch rows of its path, the crash from the recorded basis plus
//     the new slack, then the root's classification and loop.
//
// Layout (LDS, D = max_depth, m, n the canonical shape; mm = m + L rows and nn = n + L slots at level L):
//   T      (m+D+1) x pitch  slots 0..nn-1, xB in slot nn, the reduced-cost row in row mm (both move out by one per
//                           appended row); pitch odd >= n + D + 1
//   prow   n+D+1            pivot row; x of a node while it is evaluated
//   lcol   m+D+1            eta column; the crash's row permutation
//   recv, recz  D           per level: v = x_j at the branch, the node's z
//   slotvar n+D, basis m+D  as batched_two_phase.hip, with the artificial of row i keyed ART + i, ART = n + D: above
//                           every branch slack (variable n + L), so `k < nn` is the eligibility of every loop
//   recj, recf  D           per level: the branching variable; bit 0 the down side first, bit 1 the second child taken
//   pbasis  sum_{L<D} (m+L+1)  per level: the node's basis and the new slack, the crash's N for the second child
//   mipw   4 ints           the evaluation's hand-over: branching variable, its basis position
#include <cfloat>
#include <climits>

#include "device_select.hpp"
#include "lp_internal.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"

namespace {

struct MipCarve {
    int pitch;
    size_t T, prow, lcol, recv, recz, slotvar, basis, recj, recf, pbasis, mipw, bytes;   // byte offsets
};

__host__ __device__ inline MipCarve mip_carve(int m, int n, int D) {
    MipCarve k{};
    const int W = n + D + 1;
    k.pitch = (W & 1) ? W : W + 1;
    size_t o = sizeof(Published);
    k.T = o;
    o += sizeof(double) * (size_t)(m + D + 1) * k.pitch;
    k.prow = o;
    o += sizeof(double) * (size_t)W;
    k.lcol = o;
    o += sizeof(double) * (size_t)(m + D + 1);
    k.recv = o;
    o += sizeof(double) * (size_t)D;
    k.recz = o;
    o += sizeof(double) * (size_t)D;
    k.slotvar = o;
    o += sizeof(int) * (size_t)(n + D);
    k.basis = o;
    o += sizeof(int) * (size_t)(m + D);
    k.recj = o;
    o += sizeof(int) * (size_t)D;
    k.recf = o;
    o += sizeof(int) * (size_t)D;
    k.pbasis = o;
    o += sizeof(int) * ((size_t)D * (m + 1) + (size_t)D * (D - 1) / 2);
    k.mipw = o;
    o += sizeof(int) * 4;
    k.bytes = (o + 15) & ~(size_t)15;
    return k;
}

// the node's basis store of level L: sum_{l<L} (m+l+1) ints in front of it
__device__ __forceinline__ int pbasis_off(int m, int L) { return L * (m + 1) + L * (L - 1) / 2; }

__device__ __forceinline__ bool mip_beats(double z, double zs, bool maximize, double gap) {
    return maximize ? (z > zs + gap) : (z < zs - gap);
}

template <int NT>
__global__ __launch_bounds__(NT) void k_batched_mip(BatchedMipDev d) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int m0 = d.m, n0 = d.n, D = d.max_depth, ART = d.n + d.max_depth;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    const MipCarve K = mip_carve(m0, n0, D);
    const int pitch = K.pitch;
    char* base = reinterpret_cast<char*>(smem);
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = reinterpret_cast<double*>(base + K.T);
    double* prow = reinterpret_cast<double*>(base + K.prow);
    double* lcol = reinterpret_cast<double*>(base + K.lcol);
    double* recv = reinterpret_cast<double*>(base + K.recv);
    double* recz = reinterpret_cast<double*>(base + K.recz);
    int* slotvar = reinterpret_cast<int*>(base + K.slotvar);
    int* basis = reinterpret_cast<int*>(base + K.basis);
    int* recj = reinterpret_cast<int*>(base + K.recj);
    int* recf = reinterpret_cast<int*>(base + K.recf);
    int* pbasis = reinterpret_cast<int*>(base + K.pbasis);
    int* mipw = reinterpret_cast<int*>(base + K.mipw);
    int* pub = pubs->v;   // [0] entering slot / crash row, [1] leaving position, [2] singular verdict, [3] block_any

    const double* A = d.A + (size_t)lp * m0 * n0;
    const double* b = d.b + (size_t)lp * m0;
    const double* c = d.c + (size_t)lp * n0;
    const int no = d.n_orig;
    const double eps = d.eps, gap = d.gap;
    const bool maximize = d.maximize != 0;
    double* xo = d.x + (size_t)lp * no;

    if (d.run_status && d.run_status[lp] != LP_OPTIMAL) {   // (uniform over the workgroup: no barrier follows)
        for (int j = tid; j < no; j += NT) xo[j] = NAN;
        if (tid < 4) d.stats[(size_t)lp * 4 + tid] = 0;
        if (tid == 0) {
            d.obj[lp] = NAN;
            d.bound[lp] = NAN;
            d.found[lp] = 0;
            d.status[lp] = d.run_status[lp];
        }
        return;
    }
    // the current shape: the included loops read m (rows), n (slots; eligible keys are < n) and W = n + 1
    int m = m0, n = n0, W = n0 + 1;

    constexpr int ANY_WORD = 3;   // block_any's word of pub
#include "batched_block_any.hpp"

    // ---- root: T = [A | b; c | 0]; slots = the columns in order, basis = the artificials by row
    for (int s = tid; s < n0; s += NT) slotvar[s] = s;
    for (int t = tid; t < m0; t += NT) basis[t] = ART + t;
    for (int e = tid; e < m0 * n0; e += NT) {
        const int s = e / m0, i = e - s * m0;
        T[(size_t)i * pitch + s] = A[e];
    }
    for (int i = tid; i < m0; i += NT) T[(size_t)i * pitch + n0] = b[i];
    for (int j = tid; j <= n0; j += NT) T[(size_t)m0 * pitch + j] = (j < n0) ? c[j] : 0.0;
    for (int j = tid; j < no; j += NT) xo[j] = NAN;
    const int* N0 = d.basis_in + (size_t)lp * m0;
    int not_identity = 0;
    for (int e = tid; e < m0 * m0; e += NT) {
        const int t = e / m0, i = e - t * m0;
        if (A[(size_t)N0[t] * m0 + i] != ((i == t) ? 1.0 : 0.0)) not_identity = 1;
    }
    for (int t = tid; t < m0; t += NT)
        if (c[N0[t]] != 0.0) not_identity = 1;
    const bool root_identity = !block_any(not_identity);

    // ---- pivot(r, se), the primal loop simplex(phase2, maximize, iters), the dual loop dual(iters)
    constexpr bool BLAND = false;
#include "batched_lds_loop.hpp"
#include "batched_dual_loop.hpp"

    // ---- the basis install of batched_resolve.hip on the current m x n tableau
    auto crash = [&](const int* N, bool identity) __attribute__((always_inline)) -> int {
        int status = LP_OPTIMAL;
#include "batched_resolve_crash.hpp"
        if (identity) {   // the header keys the artificials n + t there: move them above the branch slacks
            for (int s = tid; s < n; s += NT)
                if (slotvar[s] >= n) slotvar[s] += ART - n;
            __syncthreads();
        }
        return status;
    };
    // ---- classification (two block reductions), then the matching loop; pivots counted per node (max_iter each)
    int nodes = 1, st_dual = 0, st_primal = 0, deepest = 0;
    auto classify_run = [&]() __attribute__((always_inline)) -> int {
        const double* drow = T + (size_t)m * pitch;
#include "batched_resolve_classify.hpp"
        int st = LP_BAD_ARG, itd = 0, itp = 0;
        if (primal_feasible)
            st = simplex(true, maximize, itp);
        else if (dual_feasible)
            st = dual(itd);
        st_dual += itd;
        st_primal += itp;
        __syncthreads();
        return st;
    };

    int st = crash(N0, root_identity);
    if (st == LP_OPTIMAL) st = classify_run();

    int status = st, found = 0;
    double zstar = 0.0, bound = NAN;
    if (st != LP_OPTIMAL) {
        if (st == LP_UNBOUNDED || st == LP_ITER_LIMIT) bound = maximize ? INFINITY : -INFINITY;
    } else {
        int L = 0, top = -1, stop = LP_OPTIMAL;
        bool have_ab = false;
        double zab = 0.0;
        for (;;) {
            bool backtrack = true;
            if (st == LP_OPTIMAL) {
                // ---- evaluate: x of the node in prow, z by thread 0 in index order, the branching variable by wave 0
                for (int j = tid; j < n; j += NT) prow[j] = 0.0;
                __syncthreads();
                for (int t = tid; t < m; t += NT) prow[basis[t]] = T[(size_t)t * pitch + n];
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
                        for (int j = 0; j < n0; ++j) z += c[j] * prow[j];
                        mipw[0] = bj == INT_MAX ? -1 : bj;
                        lcol[0] = z;
                    }
                }
                __syncthreads();
                z = lcol[0];
                const int jb = mipw[0];
                if (!found || mip_beats(z, zstar, maximize, gap)) {
                    if (jb < 0) {   // integral: the new incumbent
                        found = 1;
                        zstar = z;
                        for (int j = tid; j < no; j += NT) xo[j] = prow[j];
                    } else if (L == D) {   // fractional at the depth limit: abandoned
                        if (!have_ab || mip_beats(z, zab, maximize, 0.0)) zab = z;
                        have_ab = true;
                    } else {
                        // ---- branch: the record of level L, then the first child by appending the row
                        const double v = prow[jb];
                        const bool down = (v - floor(v)) <= 0.5;
                        int* pb = pbasis + pbasis_off(m0, L);
                        for (int t = tid; t < m; t += NT) {
                            pb[t] = basis[t];
                            if (basis[t] == jb) mipw[1] = t;
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
                        // rhs slot n -> n+1 (every row and the cost row), then the cost row m -> m+1
                        for (int i = tid; i <= m; i += NT) {
                            T[(size_t)i * pitch + n + 1] = T[(size_t)i * pitch + n];
                            T[(size_t)i * pitch + n] = 0.0;
                        }
                        __syncthreads();
                        for (int j = tid; j <= n + 1; j += NT) T[(size_t)(m + 1) * pitch + j] = T[(size_t)m * pitch + j];
                        __syncthreads();
                        for (int s = tid; s <= n + 1; s += NT) {
                            const double a = T[(size_t)t * pitch + s];
                            T[(size_t)m * pitch + s] = s < n ? (down ? -a : a)
                                                     : s == n ? 1.0 : (down ? floor(v) - v : v - ceil(v));
                        }
                        if (tid == 0) {
                            slotvar[n] = ART + m;   // the new row's artificial, barred
                            basis[m] = n0 + L;      // the slack, basic in its row
                        }
                        __syncthreads();
                        ++L;
                        m = m0 + L;
                        n = n0 + L;
                        W = n + 1;
                        ++nodes;
                        if (L > deepest) deepest = L;
                        int it = 0;
                        st = dual(it);
                        st_dual += it;
                        __syncthreads();
                        backtrack = false;
                    }
                }
            } else if (st != LP_INFEASIBLE) {
                stop = st;
                break;
            }
            if (!backtrack) continue;
            // ---- backtrack to the deepest level whose second child is pending
            while (top >= 0 && (recf[top] & 2)) --top;
            if (top < 0) break;
            __syncthreads();
            if (tid == 0) recf[top] |= 2;
            if (nodes >= d.max_nodes) {
                stop = LP_ITER_LIMIT;
                break;
            }
            // ---- the second child of level `top`: [A | 0 | b], the branch rows of its path, the recorded basis
            L = top + 1;
            m = m0 + L;
            n = n0 + L;
            W = n + 1;
            int* pb = pbasis + pbasis_off(m0, top);
            for (int e = tid; e < (m + 1) * (n + 1); e += NT) {
                const int i = e / (n + 1), j = e - i * (n + 1);
                double a = 0.0;
                if (i < m0) {
                    if (j < n0) a = A[(size_t)j * m0 + i];
                    else if (j == n) a = b[i];
                } else if (i < m) {
                    const int l = i - m0;
                    const int f = (l == top) ? (recf[l] | 2) : recf[l];
                    const bool dn = (f & 2) ? !(f & 1) : (f & 1);
                    if (j == recj[l]) a = dn ? 1.0 : -1.0;
                    else if (j == n0 + l) a = 1.0;
                    else if (j == n) a = dn ? floor(recv[l]) : -ceil(recv[l]);
                } else if (j < n0) {
                    a = c[j];
                }
                T[(size_t)i * pitch + j] = a;
            }
            for (int s = tid; s < n; s += NT) slotvar[s] = s;
            for (int t = tid; t < m; t += NT) basis[t] = ART + t;
            if (tid == 0) pb[m - 1] = n0 + top;
            __syncthreads();
            ++nodes;
            if (L > deepest) deepest = L;
            st = crash(pb, false);
            if (st == LP_OPTIMAL) st = classify_run();
        }
        __syncthreads();   // (the records tid 0 wrote last)
        // ---- status and bound (mip_ref.c step 7)
        bool have_open = have_ab;
        double zo = zab;
        for (int k = 0; k <= top; ++k)
            if (!(recf[k] & 2) || (stop != LP_OPTIMAL && k == top)) {
                if (!have_open || mip_beats(recz[k], zo, maximize, 0.0)) zo = recz[k];
                have_open = true;
            }
        if (stop != LP_OPTIMAL) status = stop;
        else if (found) status = (have_ab && mip_beats(zab, zstar, maximize, gap)) ? LP_ITER_LIMIT : LP_OPTIMAL;
        else status = have_ab ? LP_ITER_LIMIT : LP_INFEASIBLE;
        if (found) bound = (have_open && mip_beats(zo, zstar, maximize, gap)) ? zo : zstar;
        else if (have_open) bound = zo;
    }
    if (tid == 0) {
        d.status[lp] = status;
        d.found[lp] = found;
        d.obj[lp] = found ? zstar : NAN;
        d.bound[lp] = bound;
        int* so = d.stats + (size_t)lp * 4;
        so[0] = nodes;
        so[1] = st_dual;
        so[2] = st_primal;
        so[3] = deepest;
    }
}

}  // namespace

size_t lp_mip_lds_bytes(int m, int n, int max_depth) { return mip_carve(m, n, max_depth).bytes; }

bool lp_mip_fits_shape(int m, int n, int max_depth) {
    return m > 0 && n >= m && max_depth >= 0 && max_depth <= LP_MIP_MAX_DEPTH &&
           lp_mip_lds_bytes(m, n, max_depth) <= 160 * 1024;
}

int lp_batched_mip_launch(lp_context* ctx, const BatchedMipDev& d) {
    if (!lp_mip_fits_shape(d.m, d.n, d.max_depth))
        LP_FAIL(ctx, LP_BAD_ARG, "batched MIP: the shape does not fit one CU's LDS");
    // the cells of the deepest level's tableau
    return lp_launch_per_lp(ctx, (size_t)(d.m + d.max_depth + 1) * (d.n + d.max_depth + 1), k_batched_mip<256>,
                            k_batched_mip<1024>, lp_mip_lds_bytes(d.m, d.n, d.max_depth), d);
}
