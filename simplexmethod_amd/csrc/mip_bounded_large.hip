// mip_bounded_large.hip — the device side of lp_mip_bounded_solve_large: depth-first branch-and-bound over variable
// bounds on the HBM tableau of simplex_launch.hip, at any shape lp_simplex_bounded_resolve_large runs.
//
// The definition is tests/ref/mip_bounded_ref.c.  The host (simplex_bounded_driver.hip) drives the search; the tableau,
// the bound state (BoundedLargeDev), the node's lower bounds, the incumbent and the record stack stay on the device
// (MipLargeDev).  Two pieces live here:
//   staging   [A' | b' | c'] of a node from the A, b, c uploaded once per call: flagged columns and their costs
//             negated, b' the reference's two fma chains per row (the shift over lo_j != 0, then the flagged columns
//             with U_j, each in ascending j).  lp_simplex_install builds the tableau from it, so a rebuild sends no A
//             over PCIe;
//   the node  steps 3 to 5 of the reference on a node that ended LP_OPTIMAL, one workgroup: x in the caller's
//             variables, z as one serial chain on one lane, the pruning test, the branching column, and then the
//             incumbent, the abandoned node, or record L and the first child's bound change on the live tableau (one
//             held value, U_j and lo_j move).  One small result goes to pinned host memory: one host sync per node.
//
// Plain C++ and vector stores only: no inline assembly and no scalar-memory writes in this file.
#include <climits>

#include "lp_internal.hpp"
#include "simplex_problem.hpp"

namespace {

// A'[j][i] = up_j ? -A[j][i] : A[j][i] (column-major, as lp_simplex_upload stages A), and behind A' and b' the costs
// c'_j = up_j ? -c_j : c_j: one element per thread.
__global__ __launch_bounds__(256) void k_mipl_stage_columns(const double* __restrict__ A, const double* __restrict__ c,
                                                            const int* __restrict__ up, int m, int n,
                                                            double* __restrict__ As, double* __restrict__ cs) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, mn = (size_t)m * n;
    if (idx < mn) {
        const double a = A[idx];
        As[idx] = up[idx / (size_t)m] ? -a : a;
    } else if (idx < mn + n) {
        const size_t j = idx - mn;
        cs[j] = up[j] ? -c[j] : c[j];
    }
}

// b'_i: one thread per row, two chains in ascending j (mbref_install's first loop); consecutive threads read
// consecutive i of column j, and lo_j, up_j, U_j are the same for the whole block
__global__ __launch_bounds__(64) void k_mipl_stage_rhs(const double* __restrict__ A, int m, int n,
                                                       const double* __restrict__ b, const double* __restrict__ lo,
                                                       const double* __restrict__ U, const int* __restrict__ up,
                                                       double* __restrict__ bs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double acc = b[i];
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const double l = lo[j];
        if (l != 0.0) acc = fma(-A[(size_t)j * m + i], l, acc);
    }
#pragma unroll 4
    for (int j = 0; j < n; ++j)
        if (up[j]) acc = fma(-A[(size_t)j * m + i], U[j], acc);
    bs[i] = acc;
}

constexpr int kNodeThreads = 1024;
constexpr int kChunk = 4096;   // products c_j x_j staged per pass of the objective chain (32 KiB of LDS)

__device__ inline bool mipl_beats(double z, double zs, int maximize, double gap) {
    return maximize ? (z > zs + gap) : (z < zs - gap);
}

// Steps 3 to 5 of mip_bounded_ref.c on the LP_OPTIMAL tableau of a node at level L.  One workgroup; n - m, m and the
// marked columns may all exceed it, so every pass strides.
__global__ __launch_bounds__(kNodeThreads) void k_mipl_node(SimplexDev d, BoundedLargeDev bd, MipLargeDev md, int L,
                                                            int found, double zstar, int dive) {
    __shared__ double s_prod[kChunk];
    __shared__ double s_val[kNodeThreads / 64];
    __shared__ int s_idx[kNodeThreads / 64];
    __shared__ double s_z;
    __shared__ int s_go, s_jb, s_t;
    const int tid = threadIdx.x, m = d.m, n = d.n, ld = d.ld;

    // x: the basic values by position, un-complemented with U and the flags, un-shifted with the node's lo
    for (int j = tid; j < n; j += kNodeThreads) md.x[j] = 0.0;
    __syncthreads();
    for (int t = tid; t < m; t += kNodeThreads) md.x[d.basis[t]] = d.T[(size_t)t * ld + n];
    __syncthreads();
    for (int j = tid; j < n; j += kNodeThreads) {
        const double v = md.x[j], l = md.lo[j];
        const double w = bd.up[j] ? bd.U[j] - v : v;
        md.x[j] = l == 0.0 ? w : l + w;
    }
    __syncthreads();
    // z = sum c_j x_j: the products (rounded, no fma) through LDS, the sum one serial chain in index order on lane 0
    double z = 0.0;
    for (int base = 0; base < n; base += kChunk) {
        const int cnt = min(kChunk, n - base);
        for (int k = tid; k < cnt; k += kNodeThreads) s_prod[k] = md.c[base + k] * md.x[base + k];
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < cnt; ++k) z += s_prod[k];
        __syncthreads();
    }
    if (tid == 0) {
        s_z = z;
        s_go = !found || mipl_beats(z, zstar, d.maximize, md.gap);
        s_t = -1;
    }
    __syncthreads();
    z = s_z;
    MipLargeResult* res = md.result;
    if (!s_go) {   // pruned by the incumbent
        if (tid == 0) {
            res->what = LP_MIPL_PRUNED;
            res->j = -1;
            res->un_negative = 0;
            res->z = z;
            res->v = 0.0;
            __threadfence_system();
        }
        return;
    }
    // the branching column: the most fractional marked one with dist > int_tol, an exact tie to the lowest index
    // (the reference's ascending scan with a strict >)
    double best = 0.0;
    int jb = INT_MAX;
    for (int j = tid; j < md.n_orig; j += kNodeThreads) {
        if (!md.integer[j]) continue;
        const double xj = md.x[j];
        const double f = xj - floor(xj);
        const double dist = f < 1.0 - f ? f : 1.0 - f;
        if (dist > md.int_tol && dist > best) {   // j ascending per thread
            best = dist;
            jb = j;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int oj = __shfl_xor(jb, off, 64);
        if (ob > best || (ob == best && oj < jb)) {
            best = ob;
            jb = oj;
        }
    }
    if ((tid & 63) == 0) {
        s_val[tid >> 6] = best;
        s_idx[tid >> 6] = jb;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kNodeThreads / 64; ++w)
            if (s_val[w] > best || (s_val[w] == best && s_idx[w] < jb)) {
                best = s_val[w];
                jb = s_idx[w];
            }
        s_jb = jb == INT_MAX ? -1 : jb;
    }
    __syncthreads();
    jb = s_jb;
    if (jb < 0) {   // integral: the new incumbent
        for (int j = tid; j < md.n_orig; j += kNodeThreads) md.xinc[j] = md.x[j];
    } else if (L < md.max_depth) {
        // record L: the node's basis and flags (j, v, z and the side go to the host with the result)
        int* rb = md.rec_basis + (size_t)L * m;
        int* ru = md.rec_up + (size_t)L * n;
        for (int t = tid; t < m; t += kNodeThreads) {
            const int q = d.basis[t];
            rb[t] = q;
            if (q == jb) s_t = t;
        }
        for (int j = tid; j < n; j += kNodeThreads) ru[j] = bd.up[j];
    }
    __syncthreads();
    if (tid != 0) return;
    res->z = z;
    res->j = jb;
    res->un_negative = 0;
    res->v = 0.0;
    if (jb < 0) {
        res->what = LP_MIPL_INTEGRAL;
    } else if (L >= md.max_depth) {
        res->v = md.x[jb];
        res->what = LP_MIPL_ABANDONED;
    } else {
        const double v = md.x[jb];
        const int t = s_t;
        res->v = v;
        res->what = t < 0 ? LP_MIPL_NOT_BASIC : LP_MIPL_BRANCHED;
        if (t >= 0 && dive) {
            // the first child on the live tableau (step 5, the reference's operation order): the held value of
            // position t, U_j and lo_j
            double* xb = d.T + (size_t)t * ld + n;
            const int f = bd.up[jb];
            const double Uj = bd.U[jb], lj = md.lo[jb];
            double Un;
            if ((v - floor(v)) <= 0.5) {   // down: hi_j := floor(v)
                Un = floor(v) - lj;
                if (f) *xb = *xb + (Un - Uj);
            } else {                       // up: lo_j := ceil(v)
                const double dl = ceil(v) - lj;
                Un = Uj - dl;
                md.lo[jb] = lj + dl;
                if (!f) *xb = *xb - dl;
            }
            bd.U[jb] = Un;
            res->un_negative = Un < 0.0;
        }
    }
    __threadfence_system();
}

}  // namespace

void lp_mip_large_stage(lp_simplex_problem* p, const BoundedLargeDev& bd, const MipLargeDev& md) {
    const int m = p->dev.m, n = p->dev.n;
    hipStream_t s = p->ctx->stream;
    double* As = p->dT0;
    double* bs = As + (size_t)m * n;
    double* cs = bs + m;
    const size_t total = (size_t)m * n + (size_t)n;
    hipLaunchKernelGGL(k_mipl_stage_columns, (unsigned)lp_ceil_div(total, (size_t)256), 256, 0, s, md.A, md.c,
                       (const int*)bd.up, m, n, As, cs);
    hipLaunchKernelGGL(k_mipl_stage_rhs, lp_ceil_div(m, 64), 64, 0, s, md.A, m, n, md.b, (const double*)md.lo,
                       (const double*)bd.U, (const int*)bd.up, bs);
}

void lp_mip_large_node(lp_simplex_problem* p, const BoundedLargeDev& bd, const MipLargeDev& md, int L, int found,
                       double zstar, int dive) {
    hipLaunchKernelGGL(k_mipl_node, 1, kNodeThreads, 0, p->ctx->stream, p->dev, bd, md, L, found, zstar, dive);
}
