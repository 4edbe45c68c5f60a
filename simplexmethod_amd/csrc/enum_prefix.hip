// enum_prefix.hip — vertex enumeration with SHARED-PREFIX elimination over the combination
// tree (LP_ENUM_ALGO_PREFIX).  Results are bit-identical to enum_direct.hip / the oracle's
// orc_enum_subset: the per-subset solve (Gauss-Jordan with partial pivoting on the first m-2
// columns in ascending order, then a 2x2 block + back-substitution) depends, up to step t,
// only on the first t+1 columns of the subset, so all subsets sharing a prefix share that
// part of the elimination — ~O(m) flops per subset instead of O(m^3).
//
// The sorted m-subsets form a tree (depth t = t columns chosen).  A node carries the
// partially eliminated tableau restricted to the columns still selectable, [W[:, c > last] | rhs]
// (16 or 32 rows x <= n-t+1 columns), the used-row mask, min/max |pivot| and the pivot row and
// column of every depth so far.
//
//   phase 1  k_enum_expand_staged / k_enum_expand_staged32 / k_enum_expand_narrow (this file):
//            levels 0 .. D0 breadth-first through HBM (D0 = m-7 for the default second phase).
//            Wide levels: a wave per parent, staged in LDS with the subset-count table, its 16- or
//            32-lane groups (lane = row) pivot several children at a time and write the child
//            records; a block takes all its children's slots with one atomic.  Narrow levels: one
//            wave per (parent, child).  The host driver (enum_driver.hip) decides which.
//   phase 2  the leaf kernels of enum_leaf.hip (one lane per subset from the depth
//            m-7 records, with one or two more pivots done by the wave in LDS).
//   Feasible subsets are rare; each is appended to a list as (rank, record index) and its objective
//   is evaluated afterwards from that record (enum_leaf.hip: k_enum_eval_records; m = 6:
//   enum_direct.hip: k_enum_eval_list); the scored list also serves pass 2 (tie rule) without a
//   second enumeration.
//   Records have 16 rows (m <= 16) or 32 (m <= 32): the kernels below are templates over the group
//   width PGT and the column bound NMXT; <16, 16> is the tuned shape of C(32,16).
//
// Singular prefixes prune their whole subtree (min|piv| only falls, max|piv| only grows).
#include <cfloat>

#include "enum_problem.hpp"
#include "enum_tree.hpp"

namespace {

using namespace lptree;

constexpr int kExpandParents = 64;  // parents per block of k_enum_expand_staged32 (one slot allocation per block)
constexpr int kStagedParents = 256; // ... of k_enum_expand_staged (16-row records): a lane per parent in all four waves

// ---------------------------------------------------------------------------
// phase 1, wide levels of 16-row records (round 3): the PARENT RECORD STAGED IN LDS.
// The earlier form of this kernel walked a parent's children in rounds of four and fetched every operand from the
// record where it lies (HBM the first time, L2 afterwards): the pivot column, then the remaining
// columns six at a time — ~4 dependent memory round trips per round, ~20 per parent, one parent after the
// other in each wave.  PMC (scripts/pmc_kernel_bytes.py): the last level of C(32,16) moves 3.66 GB (1.14 GB
// of parents read, 2.58 GB of children written — only the columns behind a node's last chosen one are
// stored) in 1.7 ms = 2.2 TB/s: a latency chain, not a bandwidth limit.
// Here a wave copies the meaningful part of its parent (columns > last_col and the rhs: contiguous, <= 4.2 KB)
// into its private LDS slice with ONE coalesced load per lane-slot, issued one parent AHEAD (the registers
// of parent i+1 and its metadata are in flight while parent i is expanded; which part to fetch is known
// from the block's first phase, which reads every parent's last_col anyway).  Every operand of every child
// — its pivot column, the pivot row's entries (a plain LDS read at the pivot row instead of a
// ds_bpermute of the loaded column), its own entries — then comes from LDS, and the only global traffic
// inside the loop is the children's stores.  Same arithmetic, operand for operand; same slots, same
// metadata as that earlier form.  The per-level table of subset counts C(n-1-a, m-t-1) lives in LDS as well: read
// out of L2 by every parent's lane in phase A and again per lane in the expansion, those dependent little loads
// — not the records — were what a parent cost (staging the records alone changed nothing: 1.82 against 1.66 ms
// for the last level; with the table in LDS 1.04 ms = 3.5 TB/s of the 3.66 GB, the five wide levels of C(32,16)
// 2.70 -> 1.66 ms).  The child's metadata is assembled word-wise (the byte-wise form was a third of the loop's
// instructions).  A hand-counted wait for the prefetch (asm loads, s_waitcnt vmcnt(n) with n a lower bound of the
// stores issued behind them, instead of the compiler's vmcnt(0)) was tried and dropped: 1.03 against 1.04 ms.
// ---------------------------------------------------------------------------
// (4 waves per SIMD: 6 changed nothing, 8 spills and is 70 % slower)
template <int NMXT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_enum_expand_staged(EnumDev d, PrefixDev pd, int t,
                                                            const double* __restrict__ src, int src_cap,
                                                            double* __restrict__ dst, int dst_cap, int ppw, int stop,
                                                            unsigned long long begin,
                                                            unsigned long long end) {
    constexpr int PGT = 16, RS = 16, GW = 4;
    constexpr int MAXC = NMXT + PGT + 1;            // columns of a record incl. the rhs: n - t + 1 <= m + NMXT + 1
    constexpr int PER = (MAXC * RS + META + 63) / 64;   // doubles per lane that hold one record's meaningful part + metadata
    using Meta = NodeMetaT<PGT>;
    __shared__ int s_base[kStagedParents];
    __shared__ int s_last[kStagedParents];
    __shared__ int s_wtot[5];
    __shared__ __attribute__((aligned(16))) double s_rec[4][MAXC * RS + META];
    // subsets below a child with last column a: C(n-1-a, m-t-1) — one table per level, in LDS (looked up per
    // child by every parent's lane in phase A and again per lane in the expansion: out of L2 these dependent
    // little loads, not the records, were what a parent cost)
    __shared__ unsigned long long s_cnt[kEnumMaxN + 1];
    const int m = d.m, n = d.n;
    const int tid = threadIdx.x;
    if (tid <= kEnumMaxN) s_cnt[tid] = (tid < n) ? binom(d, n - 1 - tid, m - t - 1) : 0ULL;
    const int lane = tid & 63, gl = lane & (PGT - 1), g = lane / PGT, gbase = lane & ~(PGT - 1);
    const int wave = tid >> 6;
    const int nsrc = min(pd.level_counts[t], src_cap);  // (an overflowed level is reported by the host)
    const int first = blockIdx.x * 4 * ppw;
    if (first >= nsrc) return;
    // largest column expanded at depth t: the largest selectable one, n - m + t, or stop - 1 (children from column
    // `stop` on are finished from this level's records by k_enum_parent_tails, enum_leaf.hip: no slot, no store and
    // no singular count for them here; they are the last ones of their parent, so the others' rank bases stand)
    const int lim = min(n - m + t, stop - 1);
    __syncthreads();
    const size_t rdP = rec_doubles_g<PGT>(n, t, d.rs), rdC = rec_doubles_g<PGT>(n, t + 1, d.rs);
    {   // phase A: children per parent and ONE slot allocation per block — here over up to 256 parents, a lane each in
        // all four waves (the earlier form: 64 parents by one wave while three wait).  Its three dependent round trips
        // (the table above, the parents' metadata, the returning atomic: ~7 us) were a third of a 64-parent block's life.
        const int node = first + tid;
        int nch = 0, last = kHole;
        if (tid < 4 * ppw && node < nsrc) {
            const Meta* q = reinterpret_cast<const Meta*>(src + (size_t)node * rdP + (size_t)RS * (n - t + 1));
            last = q->last_col;
            if (last != kHole) {
                unsigned long long rb = q->rank_base;
                for (int a = last + 1; a <= lim; ++a) {
                    const unsigned long long cnt = s_cnt[a];
                    if (overlap(rb, cnt, begin, end) != 0ULL) ++nch;
                    rb += cnt;
                }
            }
        }
        int incl = nch;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
            for (int w = 0; w < 4; ++w) {
                const int x = s_wtot[w];
                s_wtot[w] = total;   // exclusive prefix over the waves
                total += x;
            }
            s_wtot[4] = total > 0 ? atomicAdd(&pd.level_counts[t + 1], total) : 0;
        }
        __syncthreads();
        s_base[tid] = s_wtot[4] + s_wtot[wave] + incl - nch;
        s_last[tid] = nch > 0 ? last : kHole;   // (a parent without a child in the range is skipped like a hole)
    }
    __syncthreads();
    double* L = s_rec[wave];
    double pre[PER];
    // issue the loads of this wave's parent `it` (nothing for a hole or past the end: wave-uniform)
    auto fetch = [&](int it) {
        const int local = wave * ppw + it, node = first + local;
        const int last = (it < ppw && node < nsrc) ? s_last[local] : kHole;
        if (last == kHole) return;
        const double* P = src + (size_t)node * rdP;
        const double* Q = P + (size_t)(last + 1 - t) * RS;
        const int cnt = (n - last) * RS + META;   // columns last+1 .. n-1, the rhs, and the metadata right behind it
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = u * 64 + lane;
            pre[u] = idx < cnt ? Q[idx] : 0.0;
        }
    };
    fetch(0);
    for (int it = 0; it < ppw; ++it) {
        const int local = wave * ppw + it;
        const int node = first + local;
        if (node >= nsrc) break;
        const int last = s_last[local];
        if (last == kHole) {
            fetch(it + 1);
            continue;
        }
        const int cnt = (n - last) * RS + META;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = u * 64 + lane;
            if (idx < cnt) L[idx] = pre[u];
        }
        fetch(it + 1);   // the next parent travels while this one is expanded
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nrhs = (n - 1 - last) * RS;   // offset of the rhs column inside L
        const Meta& pm = *reinterpret_cast<const Meta*>(L + nrhs + RS);   // (read from LDS where needed)
        // ---- the children, one per lane: subset counts, rank bases (exclusive scan), range overlap
        const int a_l = last + 1 + lane;
        const unsigned long long cnt_l = (a_l <= lim) ? s_cnt[a_l] : 0ULL;
        unsigned long long incl = cnt_l;
#pragma unroll
        for (int off = 1; off < (NMXT > 16 ? 64 : 32); off <<= 1) {   // at most NMXT + 1 children
            const unsigned long long o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        const unsigned long long rb_l = pm.rank_base + (incl - cnt_l);
        const unsigned long long ov_l = overlap(rb_l, cnt_l, begin, end);
        const unsigned long long vmask = __ballot(ov_l != 0ULL);
        const int nchild = __popcll(vmask);
        const int wbase = s_base[local];
        const bool prow_used = (gl >= m) || ((pm.used_mask >> gl) & 1u);
        const double prhs = L[nrhs + gl];
        unsigned long long sing = 0ULL;
        for (int k0 = 0; k0 < nchild; k0 += GW) {
            const int k = k0 + g;                  // this group's child (k-th valid one)
            const bool active = k < nchild;        // whole groups are active or not
            unsigned long long vm = vmask;
            for (int i = 0; i < (active ? k : 0); ++i) vm &= vm - 1ULL;
            const int src_lane = active ? (int)__builtin_ctzll(vm) : 0;
            const int a = last + 1 + src_lane;
            const unsigned long long rb_child = __shfl(rb_l, src_lane, 64);
            const unsigned long long ov = __shfl(ov_l, src_lane, 64);
            const int myslot = wbase + k;
            // (no wave-level operation below: groups proceed independently)
            if (!active) continue;
            if (myslot >= dst_cap) {
                if (gl == 0) atomicExch(pd.overflow, 1);
                continue;
            }
            double* C = dst + (size_t)myslot * rdC;
            Meta* cmeta = reinterpret_cast<Meta*>(C + (size_t)RS * (n - t));
            const double* La = L + (a - last - 1) * RS;   // the child's pivot column
            const double w = La[gl];
            double big;
            const int p = pick_pivot_row_g<PGT>(w, prow_used, gbase, big);
            const double minp = fmin(pm.minp, big), maxp = fmax(pm.maxp, big);
            if (!(big > 0.0) || minp <= DBL_EPSILON * (double)m * maxp) {
                sing += ov;  // the whole subtree is singular: leave a hole
                if (gl == 0) cmeta->last_col = kHole;
                continue;
            }
            const double piv = La[p];
            const double inv = 1.0 / piv;
            const bool isp = (gl == p);
            const double lx = isp ? inv : -(w * inv);
            double* Cc = C + (size_t)(a - t) * RS + gl;   // column c of the child at (c - t - 1) * RS
            const double* Lc = La + RS;                   // column a + 1 of the parent
#pragma unroll 2
            for (int c = a + 1; c < n; ++c, Lc += RS, Cc += RS) *Cc = fma(lx, Lc[p], isp ? -0.0 : Lc[gl]);
            C[(size_t)(n - t - 1) * RS + gl] = fma(lx, L[nrhs + p], isp ? -0.0 : prhs);
            if (gl == 0) {
                // the child's metadata, word-wise (64 bytes: four 16-byte stores; the pivot row / column lists
                // are the parent's with byte t patched — byte by byte this was a third of the loop's instructions)
                const uint4 pr4 = *reinterpret_cast<const uint4*>(pm.prow), pc4 = *reinterpret_cast<const uint4*>(pm.pcol);
                unsigned prw[4] = {pr4.x, pr4.y, pr4.z, pr4.w}, pcw[4] = {pc4.x, pc4.y, pc4.z, pc4.w};
                const unsigned sh = 8u * (unsigned)(t & 3), keep = ~(0xFFu << sh);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q == (t >> 2)) {
                        prw[q] = (prw[q] & keep) | ((unsigned)p << sh);
                        pcw[q] = (pcw[q] & keep) | ((unsigned)a << sh);
                    }
                uint4* out = reinterpret_cast<uint4*>(cmeta);
                const unsigned long long mn = (unsigned long long)__double_as_longlong(minp),
                                         mx = (unsigned long long)__double_as_longlong(maxp);
                out[0] = make_uint4((unsigned)rb_child, (unsigned)(rb_child >> 32), (unsigned)mn, (unsigned)(mn >> 32));
                out[1] = make_uint4((unsigned)mx, (unsigned)(mx >> 32), (unsigned)a, pm.used_mask | (1u << p));
                out[2] = make_uint4(prw[0], prw[1], prw[2], prw[3]);
                out[3] = make_uint4(pcw[0], pcw[1], pcw[2], pcw[3]);
            }
        }
        if (gl == 0 && sing) atomicAdd(&d.result->counts[2], sing);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();   // (the slice is rewritten by the next parent)
    }
}

// The staged expansion for 32-ROW records (m > 16; RS = m rounded up to even rows per column, two 32-lane groups =
// two children per wave at a time).  A record's meaningful part is up to 65 columns x 32 rows = 16.6 KB: no
// register prefetch of the next parent here (it would take 66 VGPRs) — the wave copies its parent to LDS at the
// top of each iteration, eight doubles per lane in flight at a time, and pays that one round trip per parent
// instead of the ~4 per round of the unstaged form.
template <int NMXT>
__global__ __launch_bounds__(256) void k_enum_expand_staged32(EnumDev d, PrefixDev pd, int t,
                                                              const double* __restrict__ src, int src_cap,
                                                              double* __restrict__ dst, int dst_cap, int ppw,
                                                              unsigned long long begin,
                                                              unsigned long long end) {
    constexpr int PGT = 32, GW = 2;
    constexpr int MAXC = NMXT + PGT + 1;   // columns of a record incl. the rhs: n - t + 1 <= m + NMXT + 1
    using Meta = NodeMetaT<PGT>;
    constexpr int METAD = sizeof(Meta) / 8;
    __shared__ int s_base[kExpandParents];
    __shared__ int s_last[kExpandParents];
    __shared__ __attribute__((aligned(16))) double s_rec[4][MAXC * PGT + METAD];
    __shared__ unsigned long long s_cnt[kEnumMaxN + 1];   // C(n-1-a, m-t-1) by child column a
    const int m = d.m, n = d.n;
    const int RS = rec_rs<PGT>(d.rs);
    const int tid = threadIdx.x;
    if (tid <= kEnumMaxN) s_cnt[tid] = (tid < n) ? binom(d, n - 1 - tid, m - t - 1) : 0ULL;
    const int lane = tid & 63, gl = lane & (PGT - 1), g = lane / PGT, gbase = lane & ~(PGT - 1);
    const int wave = tid >> 6;
    const int nsrc = min(pd.level_counts[t], src_cap);
    const int first = blockIdx.x * 4 * ppw;
    if (first >= nsrc) return;
    const int lim = n - m + t;
    __syncthreads();
    const size_t rdP = rec_doubles_g<PGT>(n, t, d.rs), rdC = rec_doubles_g<PGT>(n, t + 1, d.rs);
    if (tid < 64) {   // phase A (one wave: 64 parents per block)
        const int node = first + tid;
        int nch = 0, last = kHole;
        if (tid < 4 * ppw && node < nsrc) {
            const Meta* q = reinterpret_cast<const Meta*>(src + (size_t)node * rdP + (size_t)RS * (n - t + 1));
            last = q->last_col;
            if (last != kHole) {
                unsigned long long rb = q->rank_base;
                for (int a = last + 1; a <= lim; ++a) {
                    const unsigned long long cnt = s_cnt[a];
                    if (overlap(rb, cnt, begin, end) != 0ULL) ++nch;
                    rb += cnt;
                }
            }
        }
        int incl = nch;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        const int total = __shfl(incl, 63, 64);
        int base = 0;
        if (lane == 63 && total > 0) base = atomicAdd(&pd.level_counts[t + 1], total);
        base = __shfl(base, 63, 64);
        s_base[tid] = base + incl - nch;
        s_last[tid] = nch > 0 ? last : kHole;
    }
    __syncthreads();
    double* L = s_rec[wave];
    const bool row = gl < RS;   // this lane holds a row of the record
    for (int it = 0; it < ppw; ++it) {
        const int local = wave * ppw + it;
        const int node = first + local;
        if (node >= nsrc) break;
        const int last = s_last[local];
        if (last == kHole) continue;
        {   // the parent's columns last+1 .. n-1, rhs and metadata (contiguous) -> LDS, eight doubles per lane in flight
            const double* Q = src + (size_t)node * rdP + (size_t)(last + 1 - t) * RS;
            const int cnt = (n - last) * RS + METAD;
            for (int base = 0; base < cnt; base += 8 * 64) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int idx = base + u * 64 + lane;
                    v[u] = idx < cnt ? Q[idx] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int idx = base + u * 64 + lane;
                    if (idx < cnt) L[idx] = v[u];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nrhs = (n - 1 - last) * RS;
        const Meta& pm = *reinterpret_cast<const Meta*>(L + nrhs + RS);
        const int a_l = last + 1 + lane;
        const unsigned long long cnt_l = (a_l <= lim) ? s_cnt[a_l] : 0ULL;
        unsigned long long incl = cnt_l;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        const unsigned long long rb_l = pm.rank_base + (incl - cnt_l);
        const unsigned long long ov_l = overlap(rb_l, cnt_l, begin, end);
        const unsigned long long vmask = __ballot(ov_l != 0ULL);
        const int nchild = __popcll(vmask);
        const int wbase = s_base[local];
        const bool prow_used = (gl >= m) || ((pm.used_mask >> gl) & 1u);
        const double prhs = row ? L[nrhs + gl] : 0.0;
        unsigned long long sing = 0ULL;
        for (int k0 = 0; k0 < nchild; k0 += GW) {
            const int k = k0 + g;
            const bool active = k < nchild;
            unsigned long long vm = vmask;
            for (int i = 0; i < (active ? k : 0); ++i) vm &= vm - 1ULL;
            const int src_lane = active ? (int)__builtin_ctzll(vm) : 0;
            const int a = last + 1 + src_lane;
            const unsigned long long rb_child = __shfl(rb_l, src_lane, 64);
            const unsigned long long ov = __shfl(ov_l, src_lane, 64);
            const int myslot = wbase + k;
            // pick_pivot_row_g<32> exchanges between the two halves of a group: called by whole groups only, but a
            // group that is not active must still reach it together with the other one (wave-level shuffle)
            const double* La = L + (size_t)(active ? a - last - 1 : 0) * RS;
            const double w = row ? La[gl] : 0.0;
            double big;
            const int p = pick_pivot_row_g<PGT>(w, prow_used, gbase, big);
            if (!active) continue;
            if (myslot >= dst_cap) {
                if (gl == 0) atomicExch(pd.overflow, 1);
                continue;
            }
            double* C = dst + (size_t)myslot * rdC;
            Meta* cmeta = reinterpret_cast<Meta*>(C + (size_t)RS * (n - t));
            const double minp = fmin(pm.minp, big), maxp = fmax(pm.maxp, big);
            if (!(big > 0.0) || minp <= DBL_EPSILON * (double)m * maxp) {
                sing += ov;
                if (gl == 0) cmeta->last_col = kHole;
                continue;
            }
            const double piv = La[p];
            const double inv = 1.0 / piv;
            const bool isp = (gl == p);
            const double lx = isp ? inv : -(w * inv);
            double* Cc = C + (size_t)(a - t) * RS + gl;
            const double* Lc = La + RS;
            if (row) {
#pragma unroll 2
                for (int c = a + 1; c < n; ++c, Lc += RS, Cc += RS) *Cc = fma(lx, Lc[p], isp ? -0.0 : Lc[gl]);
                C[(size_t)(n - t - 1) * RS + gl] = fma(lx, L[nrhs + p], isp ? -0.0 : prhs);
            }
            if (gl == 0) {
                Meta cm = pm;   // (32-row records: 96 bytes, copied as a struct)
                cm.rank_base = rb_child;
                cm.minp = minp;
                cm.maxp = maxp;
                cm.last_col = a;
                cm.used_mask = pm.used_mask | (1u << p);
                cm.prow[t] = (unsigned char)p;
                cm.pcol[t] = (unsigned char)a;
                *cmeta = cm;
            }
        }
        if (gl == 0 && sing) atomicAdd(&d.result->counts[2], sing);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// The same expansion for NARROW levels (the first few, and every level of a small rank range):
// one WAVE per (parent, child) — lane = (row, column quarter) — with all of the child's columns
// in flight at once.  A lone 16-lane group pivoting up to n-m+1 children one after the other, four
// dependent HBM round trips per child, takes ~60 us per level: most of a small shard's run time.
template <int PGT, int NMXT>
__global__ __launch_bounds__(256) void k_enum_expand_narrow(EnumDev d, PrefixDev pd, int t,
                                                            const double* __restrict__ src, int src_cap,
                                                            double* __restrict__ dst, int dst_cap, int stop,
                                                            unsigned long long begin,
                                                            unsigned long long end) {
    const int m = d.m, n = d.n, S = n - m + 1;   // S = most children a node can have
    constexpr int GW = 64 / PGT;
    using Meta = NodeMetaT<PGT>;
    const int RS = rec_rs<PGT>(d.rs);   // row stride of the records' columns
    const int lane = threadIdx.x & 63, gl = lane & (PGT - 1), g = lane / PGT, gbase = lane & ~(PGT - 1);
    const int wid = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int node = wid / S, j = wid - node * S;
    const int nsrc = min(pd.level_counts[t], src_cap);
    if (node >= nsrc) return;
    const double* P = src + (size_t)node * rec_doubles_g<PGT>(n, t, d.rs);
    const Meta pm = *reinterpret_cast<const Meta*>(P + (size_t)RS * (n - t + 1));
    const int a = pm.last_col + 1 + j;
    if (pm.last_col == kHole || a > n - m + t || a >= stop) return;   // (stop: as in k_enum_expand_staged)
    // subsets below the siblings in front of this child: one lane per sibling and a wave sum (a loop of up to
    // n - m dependent little loads from the table in L2 was most of a narrow level's 8-60 us)
    const int a2 = pm.last_col + 1 + lane;
    unsigned long long part = (a2 < a) ? binom(d, n - 1 - a2, m - t - 1) : 0ULL;
    const unsigned long long mine = binom(d, n - 1 - a, m - t - 1);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
    const unsigned long long rb = pm.rank_base + part;
    const unsigned long long ov = overlap(rb, mine, begin, end);
    if (ov == 0ULL) return;
    int slot = 0;
    if (lane == 0) slot = atomicAdd(&pd.level_counts[t + 1], 1);
    slot = __builtin_amdgcn_readfirstlane(slot);
    if (slot >= dst_cap) {
        if (lane == 0) atomicExch(pd.overflow, 1);
        return;
    }
    double* C = dst + (size_t)slot * rec_doubles_g<PGT>(n, t + 1, d.rs);
    Meta* cmeta = reinterpret_cast<Meta*>(C + (size_t)RS * (n - t));
    const bool prow_used = (gl >= m) || ((pm.used_mask >> gl) & 1u);
    const double w = gl < RS ? P[(size_t)(a - t) * RS + gl] : 0.0;
    // this group's columns (a+1+g, a+5+g, ...; column n = the rhs): all loads issued before use
    constexpr int NC = (PGT + NMXT + 1 + GW - 1) / GW;   // n <= PGT + NMXT: at most that many columns + rhs
    double own[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const int c = a + 1 + g + GW * q;
        own[q] = (c <= n && gl < RS) ? P[(size_t)(c - t) * RS + gl] : 0.0;
    }
    double big;
    const int p = pick_pivot_row_g<PGT>(w, prow_used, gbase, big);
    const double minp = fmin(pm.minp, big), maxp = fmax(pm.maxp, big);
    if (!(big > 0.0) || minp <= DBL_EPSILON * (double)m * maxp) {
        if (lane == 0) {
            cmeta->last_col = kHole;  // the whole subtree is singular
            atomicAdd(&d.result->counts[2], ov);
        }
        return;
    }
    const int addr = (gbase + p) << 2;
    const double inv = 1.0 / bcast16(w, addr);
    const bool isp = (gl == p);
    const double lx = isp ? inv : -(w * inv);
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const int c = a + 1 + g + GW * q;
        const double pc = bcast16(own[q], addr);
        if (c <= n && gl < RS) C[(size_t)(c - t - 1) * RS + gl] = fma(lx, pc, isp ? -0.0 : own[q]);
    }
    if (lane == 0) {
        Meta cm;
        cm.rank_base = rb;
        cm.minp = minp;
        cm.maxp = maxp;
        cm.last_col = a;
        cm.used_mask = pm.used_mask | (1u << p);
        for (int k = 0; k < PGT; ++k) {
            cm.prow[k] = k == t ? (unsigned char)p : pm.prow[k];
            cm.pcol[k] = k == t ? (unsigned char)a : pm.pcol[k];
        }
        *cmeta = cm;
    }
}

// root record (depth 0): the original [A | b]
// (also resets every counter of the pass: one launch instead of two copies and four memsets,
// each of which costs a 10-30 us enqueue gap at the start of a small rank range)
template <int PGT>
__global__ void k_enum_root(EnumDev d, PrefixDev pd, double* dst) {
    const int gl = threadIdx.x;
    if (gl < 32) pd.level_counts[gl] = gl == 0 ? 1 : 0;
    if (gl == 32) {
        EnumResult r;
        r.best_key = lp_f64_key(-INFINITY);
        r.counts[0] = r.counts[1] = r.counts[2] = 0ULL;
        r.first_rank = ~0ULL;
        r.range_flag = r.pad[0] = r.pad[1] = 0ULL;
        *d.result = r;
        *pd.list_count = 0ULL;
        *pd.overflow = 0;
        pd.root_cursor[0] = pd.root_cursor[1] = 0;
        pd.item_count[0] = pd.item_count[1] = 0;
    }
    const int RS = rec_rs<PGT>(d.rs);
    if (gl >= RS) return;
    for (int c = 0; c < d.n; ++c) dst[(size_t)c * RS + gl] = gl < d.m ? d.A[gl * d.lda + c] : 0.0;
    dst[(size_t)d.n * RS + gl] = gl < d.m ? d.b[gl] : 0.0;
    if (gl == 0) {
        NodeMetaT<PGT> cm;
        cm.rank_base = 0ULL;
        cm.minp = INFINITY;
        cm.maxp = 0.0;
        cm.last_col = -1;
        cm.used_mask = 0u;
        for (int k = 0; k < PGT; ++k) cm.prow[k] = cm.pcol[k] = 0;
        *reinterpret_cast<NodeMetaT<PGT>*>(dst + (size_t)RS * (d.n + 1)) = cm;
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers (the host driver, enum_driver.hip, decides what runs)
// ---------------------------------------------------------------------------

// Root record of 16- or 32-row records (pg) into dst; also resets every counter of the pass.
void lp_enum_launch_root(lp_enum_problem* p, int pg, double* dst) {
    hipStream_t s = p->ctx->stream;
    if (pg == 32)
        hipLaunchKernelGGL(k_enum_root<32>, 1, 64, 0, s, p->dev, p->prefix, dst);
    else
        hipLaunchKernelGGL(k_enum_root<PG>, 1, 64, 0, s, p->dev, p->prefix, dst);
}

// Level t -> t+1 over the rank range [begin, end).  bound: the level's parents inside the range (exact; its holes
// among them).  Grids are sized for bound; blocks beyond the level's actual count return at once.  stop: the first
// column whose child is not expanded (n: every child is; honoured by the kernels of 16-row records).
void lp_enum_launch_level(lp_enum_problem* p, int shape, int t, bool narrow, uint64_t bound, const double* src,
                          int src_cap, double* dst, int cap, int stop, uint64_t begin, uint64_t end) {
    lp_context* ctx = p->ctx;
    hipStream_t s = ctx->stream;
    const EnumDev& d = p->dev;
    const PrefixDev& pd = p->prefix;
    const unsigned long long b = begin, e = end;
    if (narrow) {   // one wave per (parent, child)
        const unsigned grid = (unsigned)lp_ceil_div<uint64_t>(bound * (uint64_t)(d.n - d.m + 1), 4);
        if (shape == 1)
            hipLaunchKernelGGL((k_enum_expand_narrow<16, 16>), grid, 256, 0, s, d, pd, t, src, src_cap, dst, cap, stop, b, e);
        else if (shape == 2)
            hipLaunchKernelGGL((k_enum_expand_narrow<16, 57>), grid, 256, 0, s, d, pd, t, src, src_cap, dst, cap, stop, b, e);
        else
            hipLaunchKernelGGL((k_enum_expand_narrow<32, 32>), grid, 256, 0, s, d, pd, t, src, src_cap, dst, cap, d.n, b, e);
    } else if (shape == 3) {
        // 4 * ppw parents per block; ppw = 16 once that still leaves 32 waves per CU
        const int ppw = (int)std::max<uint64_t>(1, std::min<uint64_t>(kExpandParents / 4, bound / ((uint64_t)ctx->num_cus * 32)));
        const unsigned grid = (unsigned)lp_ceil_div<uint64_t>(bound, 4 * (uint64_t)ppw);
        hipLaunchKernelGGL(k_enum_expand_staged32<32>, grid, 256, 0, s, d, pd, t, src, src_cap, dst, cap, ppw, b, e);
    } else {
        // 16-row records: up to 64 parents per wave, 256 per block
        const int ppw = (int)std::max<uint64_t>(1, std::min<uint64_t>(kStagedParents / 4, bound / ((uint64_t)ctx->num_cus * 32)));
        const unsigned grid = (unsigned)lp_ceil_div<uint64_t>(bound, 4 * (uint64_t)ppw);
        if (shape == 1)
            hipLaunchKernelGGL(k_enum_expand_staged<16>, grid, 256, 0, s, d, pd, t, src, src_cap, dst, cap, ppw, stop, b, e);
        else
            hipLaunchKernelGGL(k_enum_expand_staged<57>, grid, 256, 0, s, d, pd, t, src, src_cap, dst, cap, ppw, stop, b, e);
    }
}
