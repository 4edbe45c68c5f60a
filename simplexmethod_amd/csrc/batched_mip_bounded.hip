// batched_mip_bounded.hip — depth-first BRANCH-AND-BOUND OVER VARIABLE BOUNDS for many mixed-integer LPs of one shape,
// ONE PROBLEM PER WORKGROUP.
//
// Each workgroup runs tests/ref/mip_bounded_ref.c's search with the tableau and the whole search state in LDS.  A
// branch changes one bound of the bounded-variable LP (hi_j = floor(v) or lo_j = ceil(v)), so the tableau stays
// (m+1) x (n+1) at every depth; batched_mip.hip's row form grows it by one row and one slot per level.
//   - install (the root and every second child): k_batched_bounded_resolve's load and b' chains on the node's bounds,
//     basis and flags, batched_resolve_crash.hpp, its classification and the matching loop (batched_bounded_loop.hpp,
//     batched_bounded_dual_loop.hpp);
//   - first child (dive): the branching variable is basic at position t; the new bound changes its width U_j, its shift
//     lo_j and at most the one held value xB_t, by thread 0, no pass over the tableau.  The basis stays dual feasible
//     and the bounded dual loop runs as it is;
//   - second child (rebuild): the root's lo / hi from HBM overlaid in level order with the path's records, the basis
//     and flags recorded when that level branched, then the install.
// Evaluation, incumbent, status and bound follow batched_mip.hip (mip_ref.c steps 2 and 7).
// The kernel's text is batched_mip_bounded_body.hpp, shared with k_batched_mip_bounded_long, in which every dual loop
// enters by the bound-flipping ratio test (LP_DUAL_RATIO_LONG_STEP; tests/ref/mip_bounded_long_step_ref.c).
//
// Layout (LDS): batched_bounded.hip's carve (batched_bounded_carve.hpp), then per level of max_depth D
//   recv, recz  D doubles   v = x_j at the branch, the node's z
//   recj, recf  D ints      the branching variable; bit 0 the down side first, bit 1 the second child taken
//   pbasis      D x m ints  the node's basis
//   pflags      D x FW      the node's complement flags, one bit per column, FW = ceil(n / 32) words
//   mipw        4 ints      the evaluation's hand-over: branching variable, its basis position
// Nothing per level scales with the tableau: a record is 24 + 4 m + 4 FW bytes, and max_depth goes to 1024.
#include <cfloat>
#include <climits>

#include "device_select.hpp"
#include "lp_internal.hpp"
#include "batched_problem.hpp"
#include "batched_scan.hpp"
#include "batched_bounded_carve.hpp"

namespace {

struct MipBoundedCarve {
    int fw;                                                  // flag words per level
    size_t recv, recz, recj, recf, pbasis, pflags, mipw, bytes;   // byte offsets behind the bounded carve
};

__host__ __device__ inline MipBoundedCarve mip_bounded_carve(int m, int n, int D) {
    MipBoundedCarve k{};
    k.fw = (n + 31) / 32;
    size_t o = bounded_carve(m, n).bytes;
    k.recv = o;
    o += sizeof(double) * (size_t)D;
    k.recz = o;
    o += sizeof(double) * (size_t)D;
    k.recj = o;
    o += sizeof(int) * (size_t)D;
    k.recf = o;
    o += sizeof(int) * (size_t)D;
    k.pbasis = o;
    o += sizeof(int) * (size_t)D * m;
    k.pflags = o;
    o += sizeof(int) * (size_t)D * k.fw;
    k.mipw = o;
    o += sizeof(int) * 4;
    k.bytes = (o + 15) & ~(size_t)15;
    return k;
}

__device__ __forceinline__ bool mipb_beats(double z, double zs, bool maximize, double gap) {
    return maximize ? (z > zs + gap) : (z < zs - gap);
}

// amdgpu_waves_per_eu(4): 128 VGPRs, so that four 256-thread workgroups share a CU (the compiler's own choice for that
// instantiation is 147 VGPRs and three); no scratch either way.  The kernel's text is batched_mip_bounded_body.hpp,
// shared with the _long form below.
template <int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4)))
void k_batched_mip_bounded(BatchedMipBoundedDev d) {
#include "batched_mip_bounded_body.hpp"
}

// The same search with the bound-flipping ratio test in every dual loop (LP_DUAL_RATIO_LONG_STEP,
// batched_bounded_dual_loop.hpp): the same carve, no LDS more.
template <int NT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4)))
void k_batched_mip_bounded_long(BatchedMipBoundedDev d) {
#define LP_BOUNDED_DUAL_LONG_STEP
#include "batched_mip_bounded_body.hpp"
#undef LP_BOUNDED_DUAL_LONG_STEP
}

}  // namespace

size_t lp_mip_bounded_lds_bytes(int m, int n, int max_depth) { return mip_bounded_carve(m, n, max_depth).bytes; }

bool lp_mip_bounded_fits_shape(int m, int n, int max_depth) {
    return m > 0 && n >= m && max_depth >= 0 && max_depth <= LP_MIP_BOUNDED_MAX_DEPTH && lp_bounded_fits_shape(m, n) &&
           lp_mip_bounded_lds_bytes(m, n, max_depth) <= 160 * 1024;
}

int lp_batched_mip_bounded_launch(lp_context* ctx, const BatchedMipBoundedDev& d, int dual_ratio) {
    if (!lp_dual_ratio_known(dual_ratio)) LP_FAIL(ctx, LP_BAD_ARG, "batched bounded MIP: unknown dual ratio test");
    if (!lp_mip_bounded_fits_shape(d.m, d.n, d.max_depth))
        LP_FAIL(ctx, LP_BAD_ARG, "batched bounded MIP: the shape does not fit one CU's LDS");
    if (dual_ratio == LP_DUAL_RATIO_LONG_STEP)
        return lp_launch_per_lp(ctx, (size_t)(d.m + 1) * (d.n + 1), k_batched_mip_bounded_long<256>,
                                k_batched_mip_bounded_long<1024>, lp_mip_bounded_lds_bytes(d.m, d.n, d.max_depth), d);
    return lp_launch_per_lp(ctx, (size_t)(d.m + 1) * (d.n + 1), k_batched_mip_bounded<256>, k_batched_mip_bounded<1024>,
                            lp_mip_bounded_lds_bytes(d.m, d.n, d.max_depth), d);
}
