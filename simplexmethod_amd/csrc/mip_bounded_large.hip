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
// lp_mip_bounded_solve_large_ex (tests/ref/mip_bounded_snapshots_ref.c) adds three more:
//   save      the state of a node that branched, as it was BEFORE the dive's bound change, into a snapshot slot: the
//             (m+1) x ld tableau as 16-byte moves of 64-bit words, then U and the node's lo.  The node kernel has
//             already applied the change, so it reports the three values it overwrote and where (MipLargeResult), the
//             host queues the save once it has seen LP_MIPL_BRANCHED, and the save writes those values into the slot
//             in place of the live ones: no copy for a node that does not branch, no sync of its own;
//   restore   the copy back, with the basis and the flags from the level's record (rec_basis, rec_up: the node kernel
//             recorded them before the change, so a slot does not hold them twice) and the non-basic marks set;
//   the second child   step 5 with the other side on the restored state, one workgroup: the basic columns' marks
//             cleared, the position of j found in the basis, the bound change, U' < 0 reported through the pinned
//             result.  The bounded dual loop follows where the tableau stands: no staging, crash or classification.
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
            res->t = -1;
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
    res->t = -1;
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
            // what the change overwrites, for a snapshot of the node as it stood
            res->t = t;
            res->xb_before = *xb;
            res->U_before = Uj;
            res->lo_before = lj;
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

// ---- snapshots (lp_mip_bounded_solve_large_ex)

constexpr int kCopyThreads = 256;
constexpr unsigned kCopyBlocks = 2048;   // grid-stride above this: 8 workgroups per CU

typedef unsigned long long u64;

// Saves the node into a slot.  pairs = (m+1) * ld / 2 16-byte words of the tableau (ld is a multiple of 8, both
// buffers 16-byte aligned); the 64-bit word `patch` of it (the held value of position t) is written as xb, entry j of U
// and of lo as Uj and lj: the values from before the dive's bound change.  Every index is a size_t: pairs passes 2^31
// bytes at shapes the entry accepts.
__global__ __launch_bounds__(kCopyThreads) void k_mipl_save(const ulonglong2* __restrict__ T,
                                                            ulonglong2* __restrict__ sT, size_t pairs, size_t patch,
                                                            u64 xb, const u64* __restrict__ U,
                                                            const u64* __restrict__ lo, u64* __restrict__ sU,
                                                            u64* __restrict__ slo, int n, int j, u64 Uj, u64 lj) {
    const size_t first = (size_t)blockIdx.x * kCopyThreads + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kCopyThreads;
    const size_t ppair = patch >> 1;
    for (size_t k = first; k < pairs; k += stride) {
        ulonglong2 w = T[k];
        if (k == ppair) {
            if (patch & 1) w.y = xb;
            else w.x = xb;
        }
        sT[k] = w;
    }
    for (size_t k = first; k < (size_t)n; k += stride) {
        const bool own = k == (size_t)j;
        sU[k] = own ? Uj : U[k];
        slo[k] = own ? lj : lo[k];
    }
}

// Restores a slot into the live state: the tableau, U and the node's lo from the slot, the flags and the basis from
// the level's record, every column marked non-basic (k_mipl_second_child clears the basic ones' marks).
__global__ __launch_bounds__(kCopyThreads) void k_mipl_restore(const ulonglong2* __restrict__ sT,
                                                               ulonglong2* __restrict__ T, size_t pairs,
                                                               const u64* __restrict__ sU, const u64* __restrict__ slo,
                                                               u64* __restrict__ U, u64* __restrict__ lo,
                                                               const int* __restrict__ rec_up, int* __restrict__ up,
                                                               unsigned char* __restrict__ nonbasic, int n,
                                                               const int* __restrict__ rec_basis,
                                                               int* __restrict__ basis, int m) {
    const size_t first = (size_t)blockIdx.x * kCopyThreads + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kCopyThreads;
    for (size_t k = first; k < pairs; k += stride) T[k] = sT[k];
    for (size_t k = first; k < (size_t)n; k += stride) {
        U[k] = sU[k];
        lo[k] = slo[k];
        up[k] = rec_up[k];
        nonbasic[k] = 1;
    }
    for (size_t k = first; k < (size_t)m; k += stride) basis[k] = rec_basis[k];
}

// Step 5 with the side `down` for column j of value v on a restored node, one workgroup (m may exceed it: the pass
// strides).  The result: LP_MIPL_BRANCHED with un_negative, or LP_MIPL_NOT_BASIC when the basis does not hold j.
__global__ __launch_bounds__(kNodeThreads) void k_mipl_second_child(SimplexDev d, BoundedLargeDev bd, MipLargeDev md,
                                                                    int j, double v, int down) {
    __shared__ int s_t;
    const int tid = threadIdx.x, m = d.m, n = d.n, ld = d.ld;
    if (tid == 0) s_t = -1;
    __syncthreads();
    for (int t = tid; t < m; t += kNodeThreads) {
        const int q = d.basis[t];
        d.nonbasic[q] = 0;
        if (q == j) s_t = t;
    }
    __syncthreads();
    if (tid != 0) return;
    MipLargeResult* res = md.result;
    const int t = s_t;
    res->j = j;
    res->t = t;
    res->v = v;
    res->z = 0.0;
    res->un_negative = 0;
    res->what = t < 0 ? LP_MIPL_NOT_BASIC : LP_MIPL_BRANCHED;
    if (t >= 0) {
        double* xb = d.T + (size_t)t * ld + n;
        const int f = bd.up[j];
        const double Uj = bd.U[j], lj = md.lo[j];
        double Un;
        if (down) {   // hi_j := floor(v)
            Un = floor(v) - lj;
            if (f) *xb = *xb + (Un - Uj);
        } else {      // lo_j := ceil(v)
            const double dl = ceil(v) - lj;
            Un = Uj - dl;
            md.lo[j] = lj + dl;
            if (!f) *xb = *xb - dl;
        }
        bd.U[j] = Un;
        res->un_negative = Un < 0.0;
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

size_t lp_mip_large_slot_bytes(int m, int n) {
    const size_t ld = ((size_t)n + 1 + 7) / 8 * 8, npad = ((size_t)n + 1) / 2 * 2;
    return sizeof(double) * (((size_t)m + 1) * ld + 2 * npad);
}

namespace {

struct SlotView {
    double *T, *U, *lo;
};

SlotView slot_view(const lp_simplex_problem* p, char* slot) {
    const size_t words = ((size_t)p->dev.m + 1) * (size_t)p->dev.ld, npad = ((size_t)p->dev.n + 1) / 2 * 2;
    double* T = reinterpret_cast<double*>(slot);
    return SlotView{T, T + words, T + words + npad};
}

unsigned copy_blocks(size_t pairs) {
    const size_t want = lp_ceil_div(pairs, (size_t)kCopyThreads);
    return (unsigned)(want < kCopyBlocks ? want : kCopyBlocks);
}

u64 bits_of(double v) {
    u64 w;
    std::memcpy(&w, &v, sizeof(w));
    return w;
}

}  // namespace

void lp_mip_large_save(lp_simplex_problem* p, const BoundedLargeDev& bd, const MipLargeDev& md, char* slot,
                       const MipLargeResult& r) {
    const SimplexDev& d = p->dev;
    const SlotView sv = slot_view(p, slot);
    const size_t pairs = ((size_t)d.m + 1) * (size_t)d.ld / 2;
    const size_t patch = (size_t)r.t * (size_t)d.ld + (size_t)d.n;
    hipLaunchKernelGGL(k_mipl_save, copy_blocks(pairs), kCopyThreads, 0, p->ctx->stream,
                       reinterpret_cast<const ulonglong2*>(d.T), reinterpret_cast<ulonglong2*>(sv.T), pairs, patch,
                       bits_of(r.xb_before), reinterpret_cast<const u64*>(bd.U), reinterpret_cast<const u64*>(md.lo),
                       reinterpret_cast<u64*>(sv.U), reinterpret_cast<u64*>(sv.lo), d.n, r.j, bits_of(r.U_before),
                       bits_of(r.lo_before));
}

void lp_mip_large_second_child(lp_simplex_problem* p, const BoundedLargeDev& bd, const MipLargeDev& md, char* slot,
                               int level, int j, double v, int down) {
    const SimplexDev& d = p->dev;
    const SlotView sv = slot_view(p, slot);
    const size_t pairs = ((size_t)d.m + 1) * (size_t)d.ld / 2;
    hipLaunchKernelGGL(k_mipl_restore, copy_blocks(pairs), kCopyThreads, 0, p->ctx->stream,
                       reinterpret_cast<const ulonglong2*>(sv.T), reinterpret_cast<ulonglong2*>(d.T), pairs,
                       reinterpret_cast<const u64*>(sv.U), reinterpret_cast<const u64*>(sv.lo),
                       reinterpret_cast<u64*>(bd.U), reinterpret_cast<u64*>(md.lo),
                       (const int*)(md.rec_up + (size_t)level * d.n), bd.up, d.nonbasic, d.n,
                       (const int*)(md.rec_basis + (size_t)level * d.m), d.basis, d.m);
    hipLaunchKernelGGL(k_mipl_second_child, 1, kNodeThreads, 0, p->ctx->stream, d, bd, md, j, v, down);
}
