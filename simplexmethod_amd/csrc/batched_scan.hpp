// batched_scan.hpp — wave-level pieces shared by the one-LP-per-workgroup kernels
// (batched_simplex.hip, batched_two_phase.hip): the LDS hand-over words, the order-dependent
// EPS-hysteresis scans on keyed slots (see the header comment of batched_simplex.hip) and the two
// selections of Bland's rule on keyed entries.
#pragma once

#include <cfloat>

#include "device_select.hpp"

namespace {

// Uncached-by-the-compiler LDS word accesses for the in-workgroup hand-over.  A `volatile int*` made from an LDS
// pointer is a GENERIC volatile access: the compiler emitted flat_load/flat_store with system scope (sc0 sc1) and
// waited for vmcnt and lgkmcnt — every look at the published pivot number cost hundreds of cycles.
__device__ __forceinline__ int lds_peek(const int* p) {
    int v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"((unsigned)(size_t)p) : "memory");
    return v;
}
__device__ __forceinline__ void lds_poke(int* p, int v) {
    asm volatile("ds_write_b32 %0, %1" ::"v"((unsigned)(size_t)p), "v"(v) : "memory");
}

struct Published {   // what wave 0 hands to the rest of the workgroup (first 16 bytes of LDS)
    int v[4];        // [0] entering slot, [1] leaving position
};

// The sequential EPS-hysteresis scan (SimplexSolover.h:153-161 / :164-172 / :181-192) over `count`
// (value, key) entries stored in arbitrary order; entry s is read through
// get(s, value, key, eligible).  Returns the slot of the selected entry (-1 if none) and the scan's
// final value in `best`.  Keys are the original indices: the scan order is ascending key.
//
// Done by ONE wave (the tableaus of this kernel have a few hundred rows/columns at
// most: two or three entries per lane).  No LDS scratch, no barriers; the caller publishes the
// result to the other waves.  Entries are re-read through get() on every pass.
template <bool WANT_MAX, typename Get>
__device__ int wave_scan_keyed(int count, double eps, double& best, Get get) {
    const double sentinel = WANT_MAX ? -INFINITY : INFINITY;
    const int lane = threadIdx.x & 63;
    double lv = sentinel;
    int lkey = INT_MAX, lslot = -1;
    for (int s = lane; s < count; s += 64) {
        double v;
        int k;
        bool ok;
        get(s, v, k, ok);
        if (ok && ((WANT_MAX ? (v > lv) : (v < lv)) || (v == lv && k < lkey))) {
            lv = v;
            lkey = k;
            lslot = s;
        }
    }
    // (reductions on sortable keys: device_select.hpp; lv / lp never hold a NaN — a NaN entry fails
    // every comparison above and is never taken)
    const double M = lpdev::f64_from_key(lpdev::wave_ext_key<WANT_MAX>(lpdev::f64_sort_key(lv)));
    const int jM = (int)lpdev::wave_ext_u32<false>((unsigned)((lv == M && lv != sentinel) ? lkey : INT_MAX));
    best = sentinel;
    if (jM == INT_MAX) return -1;
    const unsigned long long hit = __ballot(lv == M && lkey == jM);
    const int sM = __builtin_amdgcn_readlane(lslot, (int)__builtin_ctzll(hit));
    double lp = sentinel;
    for (int s = lane; s < count; s += 64) {
        double v;
        int k;
        bool ok;
        get(s, v, k, ok);
        if (ok && k < jM) lp = lpdev::ext2<WANT_MAX>(lp, v);
    }
    // (M beats the extreme P of the entries in front by more than eps iff it beats every lane's share
    // of them: fl(v + eps) is monotone in v — one ballot instead of a 64-bit key reduction)
    if (__ballot(!lpdev::beats<WANT_MAX>(M, lp, eps)) == 0ULL) {
        best = M;
        return sM;
    }
    // near-tie: replay the chain jump by jump (each jump: the eligible entry of smallest key beyond the threshold)
    int sel = -1;
    for (;;) {
        const double thr = WANT_MAX ? best + eps : best - eps;
        int ck = INT_MAX, cs = -1;
        double cv = 0.0;
        for (int s = lane; s < count; s += 64) {
            double v;
            int k;
            bool ok;
            get(s, v, k, ok);
            if (ok && (WANT_MAX ? (v > thr) : (v < thr)) && k < ck) {
                ck = k;
                cv = v;
                cs = s;
            }
        }
        const int kmin = (int)lpdev::wave_ext_u32<false>((unsigned)ck);
        if (kmin == INT_MAX) break;
        const int src = (int)__builtin_ctzll(__ballot(ck == kmin));
        best = lpdev::wave_bcast_f64(cv, src);
        sel = __builtin_amdgcn_readlane(cs, src);
    }
    return sel;
}

// The ratio test (:181-194) by one wave with its K = ceil(m / 64) ratios held in registers (one
// division per row instead of one per pass of wave_scan_keyed): keys are the basis positions, i.e.
// the entry index itself.  Returns the leaving position, -1 if no ratio is finite.
template <int K>
__device__ __forceinline__ int wave_ratio_select(const double (&rv)[K], int m, double eps) {
    const int lane = threadIdx.x & 63;
    double lext = INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) lext = fmin(lext, rv[k]);
    // (short-cut reductions of device_select.hpp: one 6-step pass over the high words; when a single lane
    // holds the extreme — the common case — its low word and its index come by v_readlane instead of two more passes)
    unsigned long long hit;
    const double M = lpdev::f64_from_key(lpdev::wave_ext_key_n<false, 64>(lpdev::f64_sort_key(lext), &hit));   // (fmin dropped NaNs)
    if (!(M < INFINITY)) return -1;
    int lidx = INT_MAX;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) lidx = (rv[k] == M && lane + 64 * k < m) ? lane + 64 * k : lidx;
    const int jM = ((hit & (hit - 1)) == 0ULL) ? __builtin_amdgcn_readlane(lidx, (int)__builtin_ctzll(hit))
                                               : (int)lpdev::wave_ext_u32<false>((unsigned)lidx);
    double lp = INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) lp = (lane + 64 * k < jM) ? fmin(lp, rv[k]) : lp;
    if (__ballot(!lpdev::beats<false>(M, lp, eps)) == 0ULL) return jM;   // (one ballot instead of reducing P)
    // near-tie: replay the chain jump by jump
    double best = INFINITY;
    int sel = -1;
    for (;;) {
        const double thr = best - eps;
        int cand = INT_MAX;
        double cv = INFINITY;
#pragma unroll
        for (int k = K - 1; k >= 0; --k)
            if (rv[k] < thr && lane + 64 * k < m) {
                cand = lane + 64 * k;
                cv = rv[k];
            }
        const int first = (int)lpdev::wave_ext_u32<false>((unsigned)cand);
        if (first == INT_MAX) break;
        best = lpdev::wave_bcast_f64(cv, first & 63);
        sel = first;
    }
    return sel;
}

// ---- Bland's rule (LP_PIVOT_BLAND) on keyed entries, by ONE wave (all 64 lanes) --------------------

// The eligible entry of smallest key: get(s, key, eligible).  Returns its slot, -1 if none.  Pricing
// (key = variable index, eligible = d > eps / d < -eps) and any other first-index choice.
template <typename Get>
__device__ int wave_min_key(int count, Get get) {
    const int lane = threadIdx.x & 63;
    int lkey = INT_MAX, lslot = -1;
    for (int s = lane; s < count; s += 64) {
        int k;
        bool ok;
        get(s, k, ok);
        if (ok && k < lkey) {
            lkey = k;
            lslot = s;
        }
    }
    const int kmin = (int)lpdev::wave_ext_u32<false>((unsigned)lkey);
    if (kmin == INT_MAX) return -1;
    return __builtin_amdgcn_readlane(lslot, (int)__builtin_ctzll(__ballot(lkey == kmin)));
}

// Bland's ratio test over `count` rows: get(i, theta, key) gives row i's ratio (NaN for a row outside
// R = {u_i > eps}) and the index of its basic variable.  theta* = the smallest ratio; among the rows with
// theta_i <= theta* + eps the one of smallest key leaves.  Returns the row, -1 if R is empty.  The ratios
// are computed again on the second pass (same division, same bits).
template <typename Get>
__device__ int wave_bland_ratio(int count, double eps, Get get) {
    const int lane = threadIdx.x & 63;
    double lmin = INFINITY;
    for (int i = lane; i < count; i += 64) {
        double v;
        int k;
        get(i, v, k);
        if (v < lmin) lmin = v;   // (NaN never taken)
    }
    const double thr = lpdev::f64_from_key(lpdev::wave_ext_key<false>(lpdev::f64_sort_key(lmin))) + eps;
    int lkey = INT_MAX, lrow = -1;
    for (int i = lane; i < count; i += 64) {
        double v;
        int k;
        get(i, v, k);
        if (v <= thr && k < lkey) {
            lkey = k;
            lrow = i;
        }
    }
    const int kmin = (int)lpdev::wave_ext_u32<false>((unsigned)lkey);
    if (kmin == INT_MAX) return -1;
    return __builtin_amdgcn_readlane(lrow, (int)__builtin_ctzll(__ballot(lkey == kmin)));
}

// Bland's ratio test of the bounded-variable loop: as wave_bland_ratio, with the entering variable's own candidate:
// its width ue (+inf: none) takes part in the minimum, theta* = min(min_i theta_i, ue), and, when ue <= theta* + eps,
// in the choice by smallest key with its variable index ekey.  Returns the leaving row, -2 when the entering variable
// itself wins (a bound flip), -1 when theta* = +inf (unbounded).
template <typename Get>
__device__ int wave_bland_ratio_entering(int count, double eps, double ue, int ekey, Get get) {
    const int lane = threadIdx.x & 63;
    double lmin = ue;
    for (int i = lane; i < count; i += 64) {
        double v;
        int k;
        get(i, v, k);
        if (v < lmin) lmin = v;   // (NaN never taken)
    }
    const double theta = lpdev::f64_from_key(lpdev::wave_ext_key<false>(lpdev::f64_sort_key(lmin)));
    if (!(theta < INFINITY)) return -1;
    const double thr = theta + eps;
    int lkey = (ue <= thr) ? ekey : INT_MAX, lrow = -2;
    for (int i = lane; i < count; i += 64) {
        double v;
        int k;
        get(i, v, k);
        if (v <= thr && k < lkey) {
            lkey = k;
            lrow = i;
        }
    }
    const int kmin = (int)lpdev::wave_ext_u32<false>((unsigned)lkey);
    if (kmin == INT_MAX) return -1;
    return __builtin_amdgcn_readlane(lrow, (int)__builtin_ctzll(__ballot(lkey == kmin)));
}

// ---- Devex pricing (LP_PIVOT_DEVEX) on keyed entries, by ONE wave (all 64 lanes) -------------------

// The eligible entry of largest score, exact ties to the smallest key: get(s, score, key, eligible).  Returns
// its slot, -1 if none.  Scores are >= 0 or NaN; a NaN score fails every comparison and is never taken.  No eps
// is involved, so the result does not depend on the order of the slots.
template <typename Get>
__device__ int wave_argmax_keyed(int count, Get get) {
    const int lane = threadIdx.x & 63;
    double lv = -1.0;
    int lkey = INT_MAX, lslot = -1;
    for (int s = lane; s < count; s += 64) {
        double v;
        int k;
        bool ok;
        get(s, v, k, ok);
        if (ok && (v > lv || (v == lv && k < lkey))) {
            lv = v;
            lkey = k;
            lslot = s;
        }
    }
    const double M = lpdev::f64_from_key(lpdev::wave_ext_key<true>(lpdev::f64_sort_key(lv)));
    const int kmin = (int)lpdev::wave_ext_u32<false>((unsigned)((lv == M && lslot >= 0) ? lkey : INT_MAX));
    if (kmin == INT_MAX) return -1;
    return __builtin_amdgcn_readlane(lslot, (int)__builtin_ctzll(__ballot(lv == M && lkey == kmin)));
}

}  // namespace
