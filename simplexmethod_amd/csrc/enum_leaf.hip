// enum_leaf.hip — leaf kernels of the shared-prefix enumeration: ONE LANE PER SUBSET.
//
// Input: the depth m-7 records produced breadth-first by the level kernels of enum_prefix.hip: the
// tableau [W[:, c > last] | rhs] after the first m-7 Gauss-Jordan steps, shared by every subset
// with that prefix.
//
// k_enum_leaves<1> (a third of the subsets).  A wave owns one work item (record, child column,
// chunk of subsets) at a time: it copies the record to its private LDS slice, performs the pivot
// on the child column cooperatively (16 rows x 4 columns per step; the depth m-6 tableau never
// travels through HBM; its rows are written permuted, unused rows first), and each of its 64
// lanes then finishes one subset on its own: it picks the remaining 6 columns (table of all
// 6-subsets in lexicographic order), replays the last four Gauss-Jordan steps and the 2x2 block
// exactly as oracle/lp_oracle.c: orc_enum_subset orders them, and tests feasibility.  No
// cross-lane traffic, no barriers, no divergence beyond the leaf loop's tail: the ~800
// instructions per subset are ordinary lane-parallel fp64 work, which is what this chip has in
// abundance (the cooperative sweep of enum_prefix.hip shares two more levels but is bound by the
// latency of its broadcasts, pivot searches and workgroup barriers).
//
// k_enum_leaves<3> (two thirds of the subsets).  The subsets below a child are grouped by their
// first remaining column; a group that leaves >= kGrandMin selectable columns gets a second
// in-LDS pivot and its lanes take 5 columns each (items of table 1); its large sub-groups get a
// third one (see MODE 3).  k_enum_leaves<1> finishes what is left of each child (items of table 0).
//
// k_enum_leaves_quads (table 0 of the fused path; k_enum_leaves<1> stays for m = 6 and behind LP_ENUM_LEAF_QUADS=0).
// One table entry per child; a wave pivots four children at once, a 16-lane group each, straight from the record's
// columns in registers, and its passes of 64 subsets run on from one round of children into the next.
//
// k_enum_thin (the tails).  A depth m-6 node with fewer than THIN_TAIL = 9 selectable columns holds at
// most C(8,6) = 28 subsets: as a work item it would cost a pivot and a wave pass for a handful of
// lanes, and such nodes are most of their level.  Their subsets are exactly the ones that lie
// inside the LAST 9 columns of a depth m-7 node — at most C(9,7) = 36 per record — and the tail
// kernel takes them from the records: 7 columns per lane, the lanes of a wave packed densely over
// the subsets of consecutive records, whose last columns are staged in LDS with permuted rows.
//
// k_enum_parent_tails (wide ranges).  The depth m-7 nodes with at most THIN_TAIL selectable columns — 1, 8 or 36
// subsets each, three quarters of the level — are not stored at all there: this kernel pivots them from the
// depth m-8 records, a 16-lane group per node, and finishes their subsets with the tail kernel's routine.
//
//   phase 1  the KD rows not used by the prefix x the KD chosen columns (+ rhs) sit in
//            registers; KD-2 Gauss-Jordan steps with partial pivoting among the unused rows
//            (pivot row = select chain), then the 2x2 block -> x_a, x_b.
//   phase 2  each of the m-KD rows used by the prefix streams through: KD+1 reads, the same
//            eliminations against the stored pivot rows, back-substitution, x >= -1e-9.
#include <type_traits>

#include "enum_tree.hpp"

using namespace lptree;

namespace {

constexpr int LEAF_THREADS = 256;
constexpr int LEAF_WAVES = LEAF_THREADS / 64;
#ifndef LP_GRAND_MIN
#define LP_GRAND_MIN 10
#endif
constexpr int kGrandMin = LP_GRAND_MIN;         // a depth m-5 node with >= 10 selectable columns (>= 252 subsets) is
                                      // finished by the two-level kernel (second in-LDS pivot, 5 columns per lane)
#ifndef LP_GREAT_MIN
#define LP_GREAT_MIN 9
#endif
constexpr int kGreatMin = LP_GREAT_MIN;         // k_enum_leaves<3>: a sub-group (child, j2, j3) that leaves >= 9 selectable
                                      // columns (>= 126 subsets) gets a third in-LDS pivot, 4 columns per lane
// The tail kernel (k_enum_thin) takes the subsets inside a record's last THIN_TAIL columns; children with fewer
// selectable columns leave the item tables.  C(32,16) pass with 8 / 9 / 10 columns: 12.80 / 12.67 / 14.64 ms; the
// other shapes and the shards in lp_enum_launch_leaves.
constexpr int THIN_TAIL = 9;
constexpr int TS = PG + 1;            // LDS column stride (doubles): odd, so that lanes reading the
                                      // same row of different columns hit different banks

// One subset, one lane.  tab: the node's tableau, column q (stride STRIDE doubles) = the q-th
// selectable column, column R = the rhs; c[]: the KD chosen columns; U[]: the KD rows not used by
// the prefix, ascending; used: mask of the rows the prefix did use.  PERM: the tableau's rows were
// permuted when it was written — the KD unused rows (ascending) sit at positions 0..KD-1 and the
// used ones at KD..m-1 — so every row index below is a compile-time constant (LDS reads with
// immediate offsets, pairs of rows per instruction) and U / used are ignored; the wave is then
// uniform (one tableau per wave).  Returns 0 feasible, 1 infeasible, 2 singular.
//
// OBJ (list evaluation, records in HBM): every row is finished — no early exit — and obj->z receives
// the objective, summed as the direct kernel sums it (enum_direct.hip: subset_objective): one fma per
// basis column in ascending column order, i.e. the prefix's columns (depth order), then c[0..KD-1].
struct LeafObj {
    const double* cost;           // objective coefficients by original column
    const unsigned char* prow;    // pivot row / column of each prefix depth (NodeMeta)
    const unsigned char* pcol;
    int D;                        // depth of the record
    int col0;                     // original column of tableau column 0
    unsigned used;                // PERM: rows used by the prefix (row i sits at KD + #used rows below i)
    int stride;                   // STRIDE == 0: column stride of the tableau (32-row records: EnumDev::rs)
    double z;
};

// leaf_verdict<PERM>'s row order by (step 0's pivot row p0, step 1's q1): entry p0 * KD + q1 holds the byte
// offsets (8 x row) of the KD-2 other rows, ascending, one per byte.  KD <= 6.
template <int KD>
__device__ __forceinline__ void leaf_row_table(unsigned* tab, int tid) {
    static_assert(KD <= 6, "four rows per 32-bit entry");
    if (tid < KD * KD) {
        const int p0 = tid / KD, q1 = tid - p0 * KD;
        unsigned pk = 0;
        int k = 0;
        for (int r = 0; r < KD; ++r)
            if (r != p0 && r != q1 && k < KD - 2) pk |= (unsigned)(8 * r) << (8 * k++);
        tab[tid] = pk;
    }
}

// 1.0 / x for 2^-500 <= |x| <= 2^500: the instructions the compiler emits for an f64 division without its
// range scaling (v_div_scale_f64 x 2) and special-case fix-up (v_div_fixup_f64), which leave an operand
// in that range untouched (v_div_fmas_f64 is then a plain fma, and the numerator 1.0 makes the quotient
// multiply an identity) — the same bits as `1.0 / x`, 7 instructions instead of 11
// (tests/test_gpu_enum.py::test_leaf_reciprocal_matches_division).  Outside the range: garbage, no trap.
__device__ __forceinline__ double recip_midrange(double x) {
    const double r0 = __builtin_amdgcn_rcp(x);
    const double r1 = fma(r0, fma(-x, r0, 1.0), r0);
    const double r2 = fma(r1, fma(-x, r1, 1.0), r1);
    return fma(fma(-x, r2, 1.0), r2, r2);
}
constexpr double kRecipLo = 0x1p-500, kRecipHi = 0x1p500;

// fmin / fmax of leaf_verdict's running min / max |pivot| as the instruction itself.  fmin / fmax quiet a signalling NaN
// operand first (v_max_f64 x, x) wherever the compiler cannot prove that none arrives, and it cannot for the loop-
// invariant minp0 / maxp0 of the caller, for bigs1 (the result of an asm v_max_f64) or for a value that went through the
// masked moves.  None can: minp0 / maxp0 are results of fmin / fmax over |tableau entries| in the level kernels and the
// shared pivots (or the root's constants), every `big` is a v_max_f64 result, |an fma result| or the constant -1, and the
// reciprocals are fma results — arithmetic never produces a signalling NaN.  On quiet NaNs, zeros and numbers the
// instruction is fmin / fmax bit for bit (it is what they are lowered to).
__device__ __forceinline__ double leaf_min(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double leaf_max(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The word at table[idx]: `table` is wave-uniform and held in scalar registers by the caller
// (readfirstlane of its offset), the lane's part is a 32-bit byte offset (the tables are far below 4 GB) — the load
// then takes the scalar-base form instead of a 64-bit address formed per lane.
__device__ __forceinline__ unsigned comb_word(const unsigned* table, unsigned idx) {
    return *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(table) + (size_t)(idx * 4u));
}
// A wave-uniform value that came out of memory or LDS, moved to scalar registers: what is computed from it is scalar
// arithmetic, which does not take the vector slot.
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
}
// The subsets [lo, hi) of a node whose subset 0 has rank rb, cut to the ranks inside [begin, end): hi <= lo if there is
// none.  Every operand is wave-uniform; the bounds come back in scalar registers (once per leaf
// loop, in place of two 64-bit compares and an add per lane and pass).  k_enum_leaves<0>'s form; table 1 states the
// window once per group as leaf indices and cuts with 32-bit min / max (k_enum_leaves<3> below).
__device__ __forceinline__ void clamp_to_window(unsigned long long rb, unsigned& lo, unsigned& hi, unsigned long long begin,
                                                unsigned long long end) {
    const unsigned long long rbu = uniform64(rb);
    const unsigned lou = (unsigned)__builtin_amdgcn_readfirstlane((int)lo), hiu = (unsigned)__builtin_amdgcn_readfirstlane((int)hi);
    const unsigned long long a = rbu + lou, b = rbu + hiu;
    const unsigned long long a2 = a > begin ? a : begin, b2 = b < end ? b : end;
    lo = b2 > a2 ? (unsigned)(a2 - rbu) : lou;
    hi = b2 > a2 ? (unsigned)(b2 - rbu) : lou;
}
__device__ __forceinline__ unsigned uniform_len(unsigned len) {   // (a binomial out of LDS)
    return (unsigned)__builtin_amdgcn_readfirstlane((int)len);
}
__device__ __forceinline__ unsigned uniform_off(unsigned off) {
    return (unsigned)__builtin_amdgcn_readfirstlane((int)off);
}

// d[k] = s[k], k < N, in the lanes of `mask`; the other lanes keep d.  One 64-bit move per value under the lane mask
// instead of two 32-bit selects: the mask is saved, narrowed and restored by scalar instructions, which do not take
// the vector slot the leaf kernels are bound by.  `mask` is a wave vote taken under the current lane mask, so lanes
// that are off stay off; an empty mask executes the moves as no-ops (no branch: the routine stays one basic block).
// One statement, so that nothing can be scheduled between the mask's change and its restoration; the saved mask is
// an early-clobber scalar pair of the compiler's choosing.  No s_nop stands between the mask's writes and the moves:
// the ISA's table of required software wait states lists none for a scalar write of the lane mask followed by a
// vector ALU instruction, and the compiler's own divergent blocks place none behind their s_and_saveexec_b64.
#define LP_MM_HEAD "s_and_saveexec_b64 %0, %[m]\n\t"
#define LP_MM_TAIL "s_mov_b64 exec, %0"
#define LP_MM(k) "v_mov_b64 %[d" #k "], %[s" #k "]\n\t"
#define LP_MM_D(k) [d##k] "+v"(d[k])
#define LP_MM_S(k) [s##k] "v"(s[k])
template <int N>
__device__ __forceinline__ void masked_moves(unsigned long long mask, double (&d)[N], const double (&s)[N]) {
    static_assert(N >= 4 && N <= 8, "KD - t + 1 values per row: KD <= 7, t <= KD - 3");
    unsigned long long sv;
    if constexpr (N == 4)
        asm(LP_MM_HEAD LP_MM(0) LP_MM(1) LP_MM(2) LP_MM(3) LP_MM_TAIL
            : "=&s"(sv), LP_MM_D(0), LP_MM_D(1), LP_MM_D(2), LP_MM_D(3)
            : [m] "s"(mask), LP_MM_S(0), LP_MM_S(1), LP_MM_S(2), LP_MM_S(3)
            : "scc");
    else if constexpr (N == 5)
        asm(LP_MM_HEAD LP_MM(0) LP_MM(1) LP_MM(2) LP_MM(3) LP_MM(4) LP_MM_TAIL
            : "=&s"(sv), LP_MM_D(0), LP_MM_D(1), LP_MM_D(2), LP_MM_D(3), LP_MM_D(4)
            : [m] "s"(mask), LP_MM_S(0), LP_MM_S(1), LP_MM_S(2), LP_MM_S(3), LP_MM_S(4)
            : "scc");
    else if constexpr (N == 6)
        asm(LP_MM_HEAD LP_MM(0) LP_MM(1) LP_MM(2) LP_MM(3) LP_MM(4) LP_MM(5) LP_MM_TAIL
            : "=&s"(sv), LP_MM_D(0), LP_MM_D(1), LP_MM_D(2), LP_MM_D(3), LP_MM_D(4), LP_MM_D(5)
            : [m] "s"(mask), LP_MM_S(0), LP_MM_S(1), LP_MM_S(2), LP_MM_S(3), LP_MM_S(4), LP_MM_S(5)
            : "scc");
    else if constexpr (N == 7)
        asm(LP_MM_HEAD LP_MM(0) LP_MM(1) LP_MM(2) LP_MM(3) LP_MM(4) LP_MM(5) LP_MM(6) LP_MM_TAIL
            : "=&s"(sv), LP_MM_D(0), LP_MM_D(1), LP_MM_D(2), LP_MM_D(3), LP_MM_D(4), LP_MM_D(5), LP_MM_D(6)
            : [m] "s"(mask), LP_MM_S(0), LP_MM_S(1), LP_MM_S(2), LP_MM_S(3), LP_MM_S(4), LP_MM_S(5), LP_MM_S(6)
            : "scc");
    else
        asm(LP_MM_HEAD LP_MM(0) LP_MM(1) LP_MM(2) LP_MM(3) LP_MM(4) LP_MM(5) LP_MM(6) LP_MM(7) LP_MM_TAIL
            : "=&s"(sv), LP_MM_D(0), LP_MM_D(1), LP_MM_D(2), LP_MM_D(3), LP_MM_D(4), LP_MM_D(5), LP_MM_D(6), LP_MM_D(7)
            : [m] "s"(mask), LP_MM_S(0), LP_MM_S(1), LP_MM_S(2), LP_MM_S(3), LP_MM_S(4), LP_MM_S(5), LP_MM_S(6), LP_MM_S(7)
            : "scc");
}
#undef LP_MM_HEAD
#undef LP_MM_TAIL
#undef LP_MM
#undef LP_MM_D
#undef LP_MM_S

// Rows x1 <-> x2 (three values each) in the lanes of `mask`: three 64-bit moves per value through a scratch register
// that is defined in those lanes only.
__device__ __forceinline__ void masked_row_swap(unsigned long long mask, double (&x1)[3], double (&x2)[3]) {
    unsigned long long sv;
    double tmp;
    asm("s_and_saveexec_b64 %0, %[m]\n\t"
        "v_mov_b64 %[t], %[a0]\n\tv_mov_b64 %[a0], %[b0]\n\tv_mov_b64 %[b0], %[t]\n\t"
        "v_mov_b64 %[t], %[a1]\n\tv_mov_b64 %[a1], %[b1]\n\tv_mov_b64 %[b1], %[t]\n\t"
        "v_mov_b64 %[t], %[a2]\n\tv_mov_b64 %[a2], %[b2]\n\tv_mov_b64 %[b2], %[t]\n\t"
        "s_mov_b64 exec, %0"
        : "=&s"(sv), [t] "=&v"(tmp), [a0] "+v"(x1[0]), [a1] "+v"(x1[1]), [a2] "+v"(x1[2]), [b0] "+v"(x2[0]),
          [b1] "+v"(x2[1]), [b2] "+v"(x2[2])
        : [m] "s"(mask)
        : "scc");
}

// leaf_verdict's rotation at step T: row p (T <= p < KD) of [E[:, T..KD-1] | H] moves to position T, rows T..p-1 down
// by one.  Every move of a row shares one condition — r == p for the chosen row's way into the temporaries, r <= p
// for the shift, from the highest row down — so a row is KD-T+1 moves under one mask.  Pure moves: the values and the
// order of the rows are the select form's, bit for bit.
// The masks come from the pivot search itself: eq[r] is the wave's vote on |E[r][T]| == big (a compare writes it to
// a scalar pair as it is), row r > T is the chosen one where eq[r] holds and no eq[T..r-1] does, and r <= p where some
// row holds the maximum and none of T..r-1 does (no row does if the column is all NaN: p = T, nothing moves) — scalar
// and / or / and-not on the votes in place of the select chain for p and two integer compares per row.
template <int KD, int T>
__device__ __forceinline__ void leaf_rotate_masked(double (&E)[KD][KD], double (&H)[KD], double big) {
    if constexpr (T < KD - 2) {
        constexpr int N = KD - T + 1;
        unsigned long long eq[KD], before[KD], any = 0ull;   // before[r]: a row of T..r-1 holds the maximum
#pragma unroll
        for (int r = T; r < KD; ++r) {
            eq[r] = __builtin_amdgcn_ballot_w64(fabs(E[r][T]) == big);
            before[r] = any;
            any |= eq[r];
        }
        auto get = [&](int r, double (&v)[N]) {
#pragma unroll
            for (int k = 0; k < N - 1; ++k) v[k] = E[r][T + k];
            v[N - 1] = H[r];
        };
        auto put = [&](int r, const double (&v)[N]) {
#pragma unroll
            for (int k = 0; k < N - 1; ++k) E[r][T + k] = v[k];
            H[r] = v[N - 1];
        };
        double pr[N];
        get(T, pr);
#pragma unroll
        for (int r = T + 1; r < KD; ++r) {
            double v[N];
            get(r, v);
            masked_moves<N>(eq[r] & ~before[r], pr, v);    // r == p
        }
#pragma unroll
        for (int r = KD - 1; r > T; --r) {
            double d[N], s[N];
            get(r, d);
            get(r - 1, s);
            masked_moves<N>(any & ~before[r], d, s);       // r <= p
            put(r, d);
        }
        put(T, pr);
    }
}

// Phase 2 of leaf_verdict on rows I .. END-1 of a tableau of m rows, every row index a constant: row(i, true) while a
// lane of the wave is still alive.
template <int I, int END, class Row>
__device__ __forceinline__ void leaf_rows_unrolled(int m, const bool& alive, Row& row) {
    if constexpr (I < END) {
        if (I < m && __any(alive)) {
            row(I, true);
            leaf_rows_unrolled<I + 1, END>(m, alive, row);
        }
    }
}

// FAST: every division is recip_midrange(pivot); *redo is set if a pivot of THIS function that is a number other
// than zero lay outside its range — whatever the verdict: every later pivot, and with it `sing`, then rests on
// quotients that may differ from the division's — and the caller repeats the pass with FAST = false
// (leaf_verdict below).  Tracked as maxp > 2^500 or max |1/pivot| > 2^500: a zero / NaN pivot has a NaN
// reciprocal, which v_max_f64 drops, and everything behind it is NaN as well (every later `big` stays at its
// initial -1), so the garbage behind a zero pivot — whose verdict, singular, is final and exact — never raises
// the flag; the pivots in front of the first out-of-range one are the division's bits.  (The prefix's pivots
// were divided plainly by the level kernels; a huge one, through maxp0, raises the flag all the same.)
template <int KD, int STRIDE, bool PERM, bool OBJ, bool FAST, bool TAB>
__device__ __forceinline__ int leaf_verdict_impl(const double* tab, const int (&c)[KD], int R, const int (&U)[KD],
                                                 unsigned used, double minp0, double maxp0, int m,
                                                 LeafObj* obj, bool* redo, const unsigned* rowtab) {
    auto recip = [](double x) { return FAST ? recip_midrange(x) : 1.0 / x; };
    // column stride: a template constant, or (STRIDE == 0, list evaluation from 32-row records) obj->stride
    const int S = STRIDE > 0 ? STRIDE : obj->stride;
    // ---- phase 1: unused rows x chosen columns
    double E[KD][KD], H[KD];
    // PERM (tableau in LDS): step 0's pivot row is chosen BEFORE the rows are loaded — the entries
    // are still the tableau's own, so instead of loading rows 0..KD-1 and rotating the chosen one
    // to the front (2 x (KD-1) selects per element: the largest single cost of a subset), columns
    // c[0] and c[1] are read first, and the rows then come from LDS already in their rotated
    // order: position 0 = step 0's row, position 1 = step 1's, then the other rows ascending.
    // (Not for the thin kernel's records in HBM: a second dependent round trip costs more there
    // than the selects.)
    // The same for step 1: its pivot row is the first largest entry of column c[1] AFTER step 0's
    // elimination, among the rows other than p0 — five fmas on the two columns already read (the
    // same operations, operand for operand, that step 0 performs on the loaded matrix below).
    double big0 = -1.0, bigs1 = -1.0, inv0 = 0.0;
    if constexpr (PERM) {
        double col0[KD], col1[KD];
        const double* cz = tab + c[0] * S;
        const double* cy = tab + c[1] * S;
#pragma unroll
        for (int r = 0; r < KD; ++r) {
            col0[r] = cz[r];
            col1[r] = cy[r];
        }
        int p0 = 0;
#pragma unroll
        for (int r = 0; r < KD; ++r) big0 = fmax(big0, fabs(col0[r]));
#pragma unroll
        for (int r = KD - 1; r >= 0; --r) p0 = (fabs(col0[r]) == big0) ? r : p0;   // descending: the first wins
        // the pivot element and the pivot row's entry in column c[1]: read again at the chosen row (two LDS
        // reads instead of 4 x (KD-1) selects)
        const double piv0 = cz[p0], pr01 = cy[p0];
        inv0 = recip(piv0);
        double a1[KD];
#pragma unroll
        for (int r = 0; r < KD; ++r) {
            const double u = fma(-(col0[r] * inv0), pr01, col1[r]);
            // |u|, or for row p0 some value in (-2, -1] (the high word of -1.0 over u's low word: one select
            // instead of two; all that matters is that it is negative, i.e. below every |u| and caught by the
            // `bigs1 < 0` rule below if nothing else is a number)
            a1[r] = __hiloint2double((r == p0) ? (int)0xBFF00000u : (__double2hiint(u) & 0x7FFFFFFF), __double2loint(u));
        }
        // (v_max_f64 itself: the values are |arithmetic results| or the negative marker, never signalling NaNs,
        // which the compiler cannot see behind the word-wise construction and would quiet one by one first)
#pragma unroll
        for (int r = 0; r < KD; ++r) asm("v_max_f64 %0, %1, %2" : "=v"(bigs1) : "v"(bigs1), "v"(a1[r]));
        int q1 = 0;
#pragma unroll
        for (int r = KD - 1; r >= 0; --r) q1 = (a1[r] == bigs1) ? r : q1;
        q1 = (bigs1 < 0.0) ? (p0 == 0 ? 1 : 0) : q1;   // (all NaN: any row other than p0; the subset is singular)
        // byte offsets of the rows in their rotated order: p0, q1, then the others ascending — from the
        // caller's table of all (p0, q1) pairs (leaf_row_table: one LDS read and a bit-field extract per row
        // against ~8 integer instructions per row), or computed
        unsigned off[KD];
        off[0] = (unsigned)p0 * 8u;
        off[1] = (unsigned)q1 * 8u;
        if constexpr (TAB) {
            static_assert(KD <= 6, "leaf_row_table");
            const unsigned pk = rowtab[p0 * KD + q1];
#pragma unroll
            for (int k = 0; k < KD - 2; ++k) off[k + 2] = (pk >> (8 * k)) & 0xFFu;
        } else {
            const int lo = p0 < q1 ? p0 : q1, hi = p0 < q1 ? q1 : p0;
#pragma unroll
            for (int k = 0; k < KD - 2; ++k) {
                int idx = k + (k >= lo ? 1 : 0);
                idx += (idx >= hi) ? 1 : 0;
                off[k + 2] = (unsigned)idx * 8u;
            }
        }
        auto at = [](const double* col, unsigned o) {
            return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(col) + o);
        };
#pragma unroll
        for (int t = 0; t < KD; ++t) {
            const double* col = tab + c[t] * S;
#pragma unroll
            for (int r = 0; r < KD; ++r) E[r][t] = at(col, off[r]);
        }
#pragma unroll
        for (int r = 0; r < KD; ++r) H[r] = at(tab + R * S, off[r]);
    } else {
#pragma unroll
        for (int t = 0; t < KD; ++t) {
            const double* col = tab + c[t] * S;
#pragma unroll
            for (int r = 0; r < KD; ++r) E[r][t] = col[U[r]];
        }
#pragma unroll
        for (int r = 0; r < KD; ++r) H[r] = tab[R * S + U[r]];
    }
    // Invariant: before step t, rows t..KD-1 of E are the rows not yet used, in ascending
    // original order (so "first row of largest |entry|" keeps its meaning), and rows 0..t-1
    // are the pivot rows of steps 0..t-1.  The chosen row p is ROTATED into position t
    // (rows t..p-1 move down by one): afterwards every access below has a static index —
    // no per-element "is this the pivot row" selects, and the 2x2 block is the last two rows.
    double PR[KD - 2][KD], PRH[KD - 2], INV[KD - 2];
    double minp = minp0, maxp = maxp0;
    double maxinv = 0.0;   // FAST: largest |reciprocal of a pivot| of this function
    bool sing = false;
#pragma unroll
    for (int t = 0; t < KD - 2; ++t) {
        // the largest |entry| (a NaN entry is never the maximum: fmax drops it); its first row p is found from `big`
        // by leaf_rotate_masked's votes
        double big = -1.0;
        if (PERM && t <= 1) {
            big = t == 0 ? big0 : bigs1;   // chosen while loading; the pivot rows already sit at positions 0, 1
        } else {
#pragma unroll
            for (int r = t; r < KD; ++r) big = fmax(big, fabs(E[r][t]));
        }
        // (FAST: no test here — a zero column leaves big = 0, a NaN column -1, so minp <= 0 and the threshold
        // test behind the 2x2 block says singular: one compare per step less in the leaf kernels' hot loop)
        if constexpr (!FAST) {
            if (!(big > 0.0)) sing = true;
        }
        minp = leaf_min(minp, big);
        maxp = leaf_max(maxp, big);
        // rotate row p to position t (columns t..KD-1 and the rhs).  A select on a double is two v_cndmask_b32, and
        // every select of a row shares one condition: the rows move as 64-bit moves under the lane mask
        // (leaf_rotate_masked; profiles/enum_leaf_masked_rot.json)
        const bool rotate = !(PERM && t <= 1);
        if (rotate) {
            static_assert(KD <= 7, "leaf_rotate_masked: steps 0..4");
            if (t == 0) leaf_rotate_masked<KD, 0>(E, H, big);
            else if (t == 1) leaf_rotate_masked<KD, 1>(E, H, big);
            else if (t == 2) leaf_rotate_masked<KD, 2>(E, H, big);
            else if (t == 3) leaf_rotate_masked<KD, 3>(E, H, big);
            else leaf_rotate_masked<KD, 4>(E, H, big);
        }
        // the pivot element, now in its static position (PERM, step 0: its reciprocal is already there)
        const double inv = (PERM && t == 0) ? inv0 : recip(E[t][t]);
        INV[t] = inv;
        if constexpr (FAST) maxinv = fmax(maxinv, fabs(inv));
#pragma unroll
        for (int cc = t + 1; cc < KD; ++cc) PR[t][cc] = E[t][cc];
        PRH[t] = H[t];
#pragma unroll
        for (int r = 0; r < KD; ++r) {
            if (r == t) continue;
            const double lx = -(E[r][t] * inv);
#pragma unroll
            for (int cc = t + 1; cc < KD; ++cc) E[r][cc] = fma(lx, PR[t][cc], E[r][cc]);
            H[r] = fma(lx, PRH[t], H[r]);
        }
#pragma unroll
        for (int cc = t + 1; cc < KD; ++cc) E[t][cc] = PR[t][cc] * inv;
        H[t] = PRH[t] * inv;
    }
    // ---- 2x2 block on the two rows still unused and the last two chosen columns
    const double a1 = E[KD - 2][KD - 2], a2 = E[KD - 1][KD - 2], b1 = E[KD - 2][KD - 1],
                 b2 = E[KD - 1][KD - 1], h1 = H[KD - 2], h2 = H[KD - 1];
    const bool second = fabs(a2) > fabs(a1);
    double row1[3] = {a1, b1, h1}, row2[3] = {a2, b2, h2};
    masked_row_swap(__builtin_amdgcn_ballot_w64(second), row1, row2);
    const double pa = row1[0], pb = row1[1], ph = row1[2], qa = row2[0], qb = row2[1], qh = row2[2];
    const double big1 = fabs(pa);
    const double inv1 = recip(pa);
    const double l = -(qa * inv1);
    const double wqb = fma(l, pb, qb);
    const double rq = fma(l, ph, qh);
    const double big2 = fabs(wqb);
    const double inv2 = recip(wqb);
    const double xb = rq * inv2;
    const double xa = fma(-pb, xb, ph) * inv1;
    if (!(big1 > 0.0) || !(big2 > 0.0)) sing = true;
    minp = leaf_min(minp, fmin(big1, big2));
    maxp = leaf_max(maxp, fmax(big1, big2));
    if (minp <= DBL_EPSILON * (double)m * maxp) sing = true;
    if constexpr (FAST) {
        maxinv = fmax(maxinv, fmax(fabs(inv1), fabs(inv2)));
        *redo = maxp > kRecipHi || maxinv > 1.0 / kRecipLo;
    }
    bool feas = (xa >= -1e-9) && (xb >= -1e-9);
    // the rows pivoted in phase 1: back-substitution
    double xr[OBJ ? KD - 2 : 1];
#pragma unroll
    for (int r = 0; r < KD - 2; ++r) {
        const double x = fma(-E[r][KD - 1], xb, fma(-E[r][KD - 2], xa, H[r]));
        feas = feas && (x >= -1e-9);
        if constexpr (OBJ) xr[r] = x;
    }
    // ---- phase 2: rows already used by the prefix, one at a time
    // (the loop below stops as soon as no lane of the wave is still feasible.  A lane survives phase 1 with
    // probability ~2^-KD — about one half per component: C(32,16), seed 0, has 8,102 feasible subsets of 601 M,
    // 2^-16.2 — so with six or seven columns per lane the loop usually ends after a row or two; with the four of
    // k_enum_leaves<3>'s sub-groups about four lanes of a full pass are still alive here, and it runs for about
    // three rows — 0.8 ms of a C(32,16) pass as a rolled loop: profiles/enum_leaf_defer.json)
    bool alive = !sing && feas;
    unsigned rows = used & (m >= 32 ? ~0u : ((1u << m) - 1u));
    auto one_row = [&](int i, bool has) {
        double v[KD];
#pragma unroll
        for (int t = 0; t < KD; ++t) v[t] = tab[c[t] * S + i];
        double h = tab[R * S + i];
#pragma unroll
        for (int t = 0; t < KD - 2; ++t) {
            const double lx = -(v[t] * INV[t]);
#pragma unroll
            for (int cc = t + 1; cc < KD; ++cc) v[cc] = fma(lx, PR[t][cc], v[cc]);
            h = fma(lx, PRH[t], h);
        }
        const double x = fma(-v[KD - 1], xb, fma(-v[KD - 2], xa, h));
        feas = feas && (!has || x >= -1e-9);
        alive = alive && feas;
        return x;
    };
    if constexpr (OBJ) {
        double z = 0.0;
        // (unrolled: the rows' loads of four prefix depths are in flight together — the list evaluation is one
        // lane per entry and nothing but dependent round trips to the records in HBM)
#pragma unroll 4
        for (int k = 0; k < obj->D; ++k) {
            int i = obj->prow[k];
            if constexpr (PERM) i = KD + __builtin_popcount(obj->used & ((1u << i) - 1u));
            z = fma(obj->cost[obj->pcol[k]], one_row(i, true), z);
        }
#pragma unroll
        for (int r = 0; r < KD - 2; ++r) z = fma(obj->cost[obj->col0 + c[r]], xr[r], z);
        z = fma(obj->cost[obj->col0 + c[KD - 2]], xa, z);
        z = fma(obj->cost[obj->col0 + c[KD - 1]], xb, z);
        obj->z = z;
    } else if constexpr (PERM && TAB) {
        // (the tuned kernels, tableaus of PG rows: unrolled over the rows the tableau can hold, so that every row is an
        // LDS read at an immediate offset from the column addresses phase 1 already holds — the rolled loop spends ten
        // of its ~26 vector instructions per row on addresses: a running pointer per column and an add per read)
        // (by recursion: the compiler does not unroll a loop that leaves through a wave vote)
        static_assert(STRIDE == PG + 1, "rows of a tableau in LDS");
        leaf_rows_unrolled<KD, PG>(m, alive, one_row);
    } else if constexpr (PERM) {
        for (int i = KD; i < m && __any(alive); ++i) one_row(i, true);
    } else {
        while (__any(alive && rows != 0u)) {
            const bool has = rows != 0u;
            const int i = has ? __builtin_ctz(rows) : 0;
            rows &= rows - 1u;
            one_row(i, has);
        }
    }
    return sing ? 2 : (feas ? 0 : 1);
}

// FAST: the leaf kernels' hot form.  A subset whose pivots leave recip_midrange's range (and that is not
// singular anyway) raises *viol; the kernel then sets EnumResult::range_flag, and the host repeats the pass
// on the EXACT instantiations of the kernels (plain divisions; enum_driver.hip: prefix_range).  Only
// a problem scaled to ~1e-150 or ~1e150 as a whole gets there: a non-singular subset's pivots lie within
// 1/(eps m) = 2^48 of each other.  (Repeating the one subset in place — the exact form inlined behind the
// fast one, or called — cost the leaf loops 50-200 bytes of spills and the thin kernel a wave per SIMD.)
template <int KD, int STRIDE, bool PERM, bool OBJ = false, bool FAST = false, bool TAB = false>
__device__ __forceinline__ int leaf_verdict(const double* tab, const int (&c)[KD], int R, const int (&U)[KD],
                                            unsigned used, double minp0, double maxp0, int m,
                                            LeafObj* obj = nullptr, unsigned* viol = nullptr,
                                            const unsigned* rowtab = nullptr) {
    static_assert(!(OBJ && FAST), "the list evaluation divides plainly");
    bool redo = false;
    const int v = leaf_verdict_impl<KD, STRIDE, PERM, OBJ, FAST, TAB>(tab, c, R, U, used, minp0, maxp0, m, obj, &redo, rowtab);
    if constexpr (FAST) *viol |= redo ? 1u : 0u;
    return v;
}

#ifdef LP_LEAF_WAVELOG
// Diagnostic build (scripts/leaf_wavelog.py): every wave of the leaf kernels leaves {kernel, hardware id, start,
// first item, end (100 MHz clock), items, steals}; read back through lp_debug_leaf_wavelog.
constexpr int kWaveLogCap = 1 << 16;
__device__ unsigned long long g_wavelog[kWaveLogCap][6];
__device__ unsigned int g_wavelog_n;
__device__ __forceinline__ void wavelog_put(int kernel, unsigned long long t0, unsigned long long t1, unsigned int items,
                                            unsigned int steals) {
    if ((threadIdx.x & 63) == 0) {
        const unsigned int k = atomicAdd(&g_wavelog_n, 1u);
        if (k < (unsigned)kWaveLogCap) {
            unsigned int hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            g_wavelog[k][0] = (unsigned long long)kernel | ((unsigned long long)blockIdx.x << 8);
            g_wavelog[k][1] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
            g_wavelog[k][2] = t0;
            g_wavelog[k][3] = t1;
            g_wavelog[k][4] = __builtin_amdgcn_s_memrealtime();
            g_wavelog[k][5] = (unsigned long long)items | ((unsigned long long)steals << 32);
        }
    }
}
#endif

constexpr int kChunk = 1024;  // subsets per work item (16 wave passes)
// Table 1 (k_enum_leaves<3>) on a range of at least kChunkWideMinRecords depth m-7 records: items of kChunkWide subsets.
// Every item of a large group repeats the child pivot and the j2 pivot.  C(32,16) pass with 1024 / 2048 / 4096 (wall,
// means of 3 x 12 on one MI355X, profiles/enum_leaf_steps.json): 12.69 / 12.59 / 12.62 ms.  A small range keeps 1024:
// forced to 2048 / 4096, C(28,14) takes 1.160 / 1.184 ms against 1.137 and the slowest 8-way shard of C(32,16) 1.980 /
// 2.081 ms against 1.955 (the last items of the table decide when such a pass ends) — the threshold is the one of
// kItemLanesNarrow, between those two ranges (116 k and 250 k records) and a whole C(32,16) (2.0 M).
constexpr int kChunkWide = 2048, kChunkWideMinRecords = 300000;
// lanes of k_enum_make_items that share one record: 4 on wide levels, 8 on the narrow ones of a small
// rank range (there the kernel's run time is the length of one lane's loop)
constexpr int kItemLanesWide = 4, kItemLanesNarrow = 8;

// Work items of the leaf kernels, so that no item is longer than 16 wave passes — a depth m-6 node
// can hold up to C(22,6) = 74,613 subsets, and a rank-range shard of an 8-GPU run is only a few
// milliseconds of work in total.  One lane per record; slots in the item tables are allocated with
// one atomic per wave and table.  FUSED: records are depth m-7 nodes; for each child a (with at
// least min_child_R selectable columns; the thin kernel takes the rest) whose subsets meet
// [begin, end):
//   table 1 (k_enum_leaves<3>): the child's subsets are grouped by their first remaining column
//     j2 (lexicographic order); every group that leaves at least kGrandMin selectable columns is
//     cut into items (record, a | j2 << 8 | groups << 16, first subset of the chunk inside the
//     group, rank offset of the group inside the record) — a large group in chunks of kChunk, or
//     several consecutive small groups packed into one item;
//   table 0 (k_enum_leaves<1>): the child's remaining subsets — (record, a, first subset of the
//     chunk inside the child, rank offset of the child inside the record).  `quads` (k_enum_leaves_quads): one
//     entry per child; else children 2k and 2k+1 of a record share an item.
// !FUSED (m = 6): the one record is the depth m-6 root itself, table 0 only.
template <bool FUSED>
__global__ __launch_bounds__(1024) void k_enum_make_items(EnumDev d, PrefixDev pd,
                                                         const double* __restrict__ roots,
                                                         int root_level, int root_cap, int min_child_R,
                                                         int kItemLanes, int chunk1, int quads,
                                                         unsigned long long begin, unsigned long long end) {
    constexpr int KD = 6;
    const unsigned long long kChunk1 = (unsigned long long)chunk1;   // width of a table-1 item (kChunk or a multiple)
    // C(r, 5) and C(r, 6) for r <= NMX + KD + 1, from LDS (the loops below are chains of dependent
    // lookups; out of L2 they were half of this kernel's time)
    __shared__ unsigned int s_b5[NMX + KD + 2], s_b6[NMX + KD + 2];
    if (threadIdx.x < NMX + KD + 2) {
        s_b5[threadIdx.x] = (unsigned int)d.binom[threadIdx.x * kBinomK + KD - 1];
        s_b6[threadIdx.x] = (unsigned int)d.binom[threadIdx.x * kBinomK + KD];
    }
    __syncthreads();
    // s_n1[R]: table-1 items of a child with R selectable columns whose whole rank interval lies inside
    // [begin, end) — the count pass below then costs such a child one lookup instead of the group loop
    // (nearly every child of a pass is one; the count pass was ~40 % of this kernel, which is 10 % of
    // an 8-way shard's run time)
    __shared__ int s_n1[NMX + KD + 2];
    if (threadIdx.x < NMX + KD + 2) {
        const int R = threadIdx.x;
        int n1 = 0, pack_ng = 0;
        unsigned long long pack_n = 0;
        for (int j2 = 0; R - 1 - j2 >= kGrandMin; ++j2) {
            const unsigned long long cnt2 = s_b5[R - 1 - j2];
            if (cnt2 >= kChunk1) {
                n1 += pack_ng ? 1 : 0;
                pack_ng = 0;
                pack_n = 0;
                n1 += (int)((cnt2 + kChunk1 - 1) / kChunk1);
            } else {
                if (pack_n + cnt2 > kChunk1) {
                    n1 += pack_ng ? 1 : 0;
                    pack_ng = 0;
                    pack_n = 0;
                }
                ++pack_ng;
                pack_n += cnt2;
            }
        }
        s_n1[R] = n1 + (pack_ng ? 1 : 0);
    }
    __syncthreads();
    const int n = d.n, m = d.m, D = m - KD - (FUSED ? 1 : 0);
    const int nroots = min(pd.level_counts[root_level], root_cap);
    // kItemLanes lanes share a record: lane `sub` takes the children sub, sub + kItemLanes, ... (the
    // order of the items in the tables does not matter)
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int rec = FUSED ? gid / kItemLanes : gid, sub = FUSED ? gid % kItemLanes : 0;
    const int lane = threadIdx.x & 63;
    int last = kHole;
    unsigned long long rb0 = 0ULL;
    if (rec < nroots) {
        const NodeMeta* pm = reinterpret_cast<const NodeMeta*>(roots + (size_t)rec * rec_doubles(n, D) +
                                                               (size_t)PG * (n - D + 1));
        last = pm->last_col;
        rb0 = pm->rank_base;
    }
    // chunks of [lo0, hi0) (subset indices relative to `base`) whose rank interval meets [begin, end)
    auto chunks = [&](unsigned long long base, unsigned long long lo0, unsigned long long hi0, unsigned long long ck, auto&& f) {
        for (unsigned long long lo = lo0; lo < hi0; lo += ck)
            if (overlap(base + lo, (hi0 - lo < ck) ? hi0 - lo : ck, begin, end)) f((int)lo);
    };
    // one child a (R selectable columns, L subsets from rank rb) of this lane's share
    auto child = [&](int a, int R, unsigned long long L, unsigned long long rb, int lim, auto&& emit) {
        // groups j2 = 0, 1, ... with at least kGrandMin columns left; consecutive small
        // groups are packed into one item (the child pivot is paid once per item)
        unsigned long long off2 = 0, pack_off = 0, pack_n = 0;
        int pack_j2 = 0, pack_ng = 0;
        auto flush = [&]() {
            if (pack_ng && overlap(rb + pack_off, pack_n, begin, end))
                emit(1, a | (pack_j2 << 8) | (pack_ng << 16), 0, (int)(rb + pack_off - rb0));
            pack_ng = 0;
            pack_n = 0;
        };
        for (int j2 = 0; R - 1 - j2 >= kGrandMin; ++j2) {
            const unsigned long long cnt2 = s_b5[R - 1 - j2];
            if (cnt2 >= kChunk1) {
                flush();
                chunks(rb + off2, 0, cnt2, kChunk1,
                       [&](int lo) { emit(1, a | (j2 << 8) | (1 << 16), lo, (int)(rb + off2 - rb0)); });
            } else {
                if (pack_n + cnt2 > kChunk1) flush();
                if (pack_ng == 0) {
                    pack_j2 = j2;
                    pack_off = off2;
                }
                ++pack_ng;
                pack_n += cnt2;
            }
            off2 += cnt2;
        }
        flush();
        // table 0: what is left of the child, [off2, L) — at most C(kGrandMin, 6) subsets.
        // Children 2k and 2k+1 of a record share one item (k_enum_leaves<1> pivots both
        // from the one record and fills its passes from both tails), emitted by the even one.
        const bool odd = (a - last - 1) & 1;
        const bool mine = overlap(rb + off2, L - off2, begin, end) != 0ULL;
        if (quads) {   // one entry per child; a lane's children stay adjacent in the table
            if (mine) emit(0, a, (int)off2, (int)(rb - rb0));
            return;
        }
        bool partner = false;   // does the other child of the pair exist and overlap?
        if (!odd && a + 1 <= lim && n - 2 - a >= min_child_R) {
            const int Rn = R - 1;
            unsigned long long offn = 0;
            for (int j2 = 0; Rn - 1 - j2 >= kGrandMin; ++j2) offn += s_b5[Rn - 1 - j2];
            partner = overlap(rb + L + offn, s_b6[Rn] - offn, begin, end) != 0ULL;
        }
        if (odd) {
            // (its tail rides in the even child's item: that one is emitted whenever either
            // tail meets the range)
        } else if (mine || partner) {
            emit(0, a | (partner ? 1 << 16 : 0), (int)off2, (int)(rb - rb0));
        }
    };
    // COUNT: only the number of items per table is wanted — a child whose whole interval lies inside
    // the range takes its table-1 count from s_n1 and (even children) one table-0 item
    auto visit = [&](auto&& emit, auto count_only) {   // emit(table, a_field, first subset, rank offset)
        if (last == kHole) return;
        if (FUSED) {
            unsigned long long rb = rb0;
            const int lim = n - m + D;  // largest column selectable at depth D
            for (int a = last + 1; a <= lim; ++a) {
                const int R = n - 1 - a;
                const unsigned long long L = s_b6[R];
                if (R >= min_child_R && ((a - last - 1) >> 1) % kItemLanes == sub) {
                    if (decltype(count_only)::value && rb >= begin && rb + L <= end) {
                        for (int k = 0; k < s_n1[R]; ++k) emit(1, 0, 0, 0);
                        if (quads || !((a - last - 1) & 1)) emit(0, 0, 0, 0);
                    } else {
                        child(a, R, L, rb, lim, emit);
                    }
                }
                rb += L;
            }
        } else {
            chunks(rb0, 0, s_b6[n - 1 - last], (unsigned long long)kChunk, [&](int lo) { emit(0, last, lo, 0); });
        }
    };
    int nch[2] = {0, 0};
    visit([&](int tab, int, int, int) { ++nch[tab]; }, std::true_type{});
    // slots: wave scan, then ONE atomic per block and table (a returning atomic on one word costs
    // ~11 ns chip-wide; at one per wave they were most of this kernel's time)
    __shared__ int s_wave_total[2][16], s_block_base[2];
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    int at[2];
#pragma unroll
    for (int tab = 0; tab < 2; ++tab) {
        int incl = nch[tab];   // inclusive wave scan
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) s_wave_total[tab][wave] = incl;
        at[tab] = incl - nch[tab];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int tab = threadIdx.x;
        int total = 0;
        for (int w = 0; w < nwaves; ++w) {
            const int t = s_wave_total[tab][w];
            s_wave_total[tab][w] = total;   // exclusive prefix over the waves
            total += t;
        }
        s_block_base[tab] = total ? atomicAdd(&pd.item_count[tab], total) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int tab = 0; tab < 2; ++tab) at[tab] += s_block_base[tab] + s_wave_total[tab][wave];
    visit([&](int tab, int a, int lo, int roff) {
        int4* items = tab ? pd.items2 : pd.items;
        const int cap = tab ? pd.item_cap2 : pd.item_cap;
        const int k = tab ? at[1]++ : at[0]++;
        if (k < cap) items[k] = make_int4(rec, a, lo, roff);
    }, std::false_type{});
}

// MODE 1: work items of table 0 over the depth m-7 records; the wave pivots on the child column
//         itself (depth m-6 tableau in LDS), the lanes take the 6 remaining columns.
// MODE 3: work items of table 1; the wave pivots twice (child, then the group's first column j2:
//         depth m-5 tableau in LDS) and the lanes take the 5 remaining columns — consecutive
//         subsets share their first remaining column and with it the whole first elimination
//         step, which costs a lane a third of its instructions.  A kernel of its own so that the
//         register allocation of MODE 1's loop is not disturbed (the two loops in one kernel cost
//         that loop 12 %).
//         Inside a group the subsets are in lexicographic order again, so those that share their
//         first remaining column j3 are consecutive — C(R2 - 1 - j3, 4) of them.  Every such sub-group that leaves
//         >= kGreatMin selectable columns (half of all subsets of C(32,16)) gets a THIRD in-LDS pivot and its lanes
//         take 4 columns each (two Gauss-Jordan steps whose rows are chosen before they are loaded, no register
//         rotation at all, then the 2x2 block: ~200 instructions per subset against ~320 with 5 columns); what is
//         left of the group is finished with 5 columns.  The great-grandchild tableau lives in the
//         half of the record's double buffer that the NEXT item's record will be written to (free until then).
// MODE 0 (m = 6): the root record is the depth m-6 node.
// (No MODE 2: it was MODE 3 without the third pivot; tests and profiles name the others by these numbers.)
template <int MODE, bool EXACT>
__global__ __launch_bounds__(LEAF_THREADS) __attribute__((amdgpu_waves_per_eu(3)))
void k_enum_leaves(EnumDev d, PrefixDev pd, const double* __restrict__ roots, int chunk1, unsigned long long begin,
                   unsigned long long end) {
    constexpr bool FUSED = MODE != 0;
    // subsets per work item: table 1's width is the host's choice (lp_enum_launch_leaves), the one its items were cut at
    const unsigned int width = MODE == 3 ? (unsigned int)chunk1 : (unsigned int)kChunk;
    constexpr int KD = 6;
    constexpr int MAXCOLS = NMX + KD + 1 + (FUSED ? 1 : 0);  // columns of a record (+ rhs)
    constexpr int CHILDCOLS = NMX + KD + 1;                  // columns of a depth m-6 tableau (+ rhs)
    __shared__ __attribute__((aligned(16))) double s_tab[LEAF_WAVES * 2][MAXCOLS * TS];  // double-buffered
    __shared__ __attribute__((aligned(16))) double s_child[FUSED ? LEAF_WAVES : 1][FUSED ? CHILDCOLS * TS : 1];
    __shared__ __attribute__((aligned(16))) double s_child2[MODE == 1 ? LEAF_WAVES : 1][MODE == 1 ? CHILDCOLS * TS : 1];
    __shared__ __attribute__((aligned(16))) double s_grand[MODE == 3 ? LEAF_WAVES : 1][MODE == 3 ? (NMX + KD) * TS : 1];
    __shared__ unsigned int s_binom[(NMX + KD + 2) * (KD + 1)];  // C(r, k), r <= NMX+KD+1, k <= KD
    __shared__ unsigned long long s_cnt[3];
    __shared__ unsigned int s_off[32];  // offsets of the per-R subset tables inside pd.comb6
    __shared__ unsigned int s_rows[36];  // leaf_row_table of this kernel's lanes (5 columns each in MODE 3, else 6)
    __shared__ unsigned int s_off4[MODE == 3 ? 32 : 1], s_rows4[MODE == 3 ? 16 : 1];   // MODE 3: the same for 4 columns
    __shared__ unsigned long long s_run[LEAF_WAVES];   // every wave's run of work items {next, end}: see draw() below
    __shared__ int s_dry;                              // a wave of this workgroup has seen the end of the item table

    const int m = d.m, n = d.n, D = m - KD - (FUSED ? 1 : 0);   // depth of the records
    const int4* const items = MODE == 3 ? pd.items2 : pd.items;   // built by k_enum_make_items
    const int nitems = MODE == 3 ? min(pd.item_count[1], pd.item_cap2) : min(pd.item_count[0], pd.item_cap);
    int* const cursor = pd.root_cursor + (MODE == 3 ? 1 : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef LP_LEAF_WAVELOG
    const unsigned long long wl_t0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long wl_t1 = 0;
    unsigned int wl_items = 0, wl_steals = 0;
#endif
    for (int k = tid; k < (NMX + KD + 2) * (KD + 1); k += LEAF_THREADS) {
        const int r = k / (KD + 1), kk = k - r * (KD + 1);
        s_binom[k] = (unsigned int)d.binom[r * kBinomK + kk];
    }
    if (tid < 3) s_cnt[tid] = 0ULL;
    if (tid < 32) s_off[tid] = MODE == 3 ? pd.comb5[tid] : pd.comb6[tid];
    leaf_row_table<(MODE == 3 ? 5 : 6)>(s_rows, tid);
    if constexpr (MODE == 3) {
        if (tid < 32) s_off4[tid] = pd.comb4[tid];
        leaf_row_table<4>(s_rows4, tid);
    }
    __syncthreads();
    unsigned int cntF = 0, cntI = 0, cntS = 0;
    unsigned int viol = 0;   // !EXACT: a pivot left the fast reciprocal's range (leaf_verdict)

    // Software pipeline over work items: while item A is computed from LDS slice `buf`, the whole
    // record of item B (its index was drawn one iteration earlier) is in flight into registers,
    // and the index of item C is being drawn — neither the atomic nor the HBM round trip of a
    // record sits between two items.
    constexpr int NLOAD = (MAXCOLS * PG + 63) / 64;   // doubles per lane to hold one record
    const int rec_cols = n - D + 1;                   // columns of a record incl. rhs
    // Items are dealt in runs of kRun: one returning atomic on a single word costs ~11 ns chip-wide, which at one
    // draw per item bounds the kernel.  The first deal is static — wave w owns items [w*k0, (w+1)*k0) — so that
    // the launch does not open with two atomics per wave on that word (~0.2 ms for a full grid).
    // A wave's run lives in LDS as one 64-bit word {next item, end of the run}, and items leave it by compare-and-
    // swap: when the table is dealt out, a wave that has nothing left takes items out of the runs of the other
    // waves of its workgroup (a workgroup's wave slots and LDS are free for the next kernel's blocks only when its
    // LAST wave ends).  That is what lets the runs stay at kRun to the end: rounds 1-3 shrank them with what was
    // left (guided self-scheduling), and the last ~4 items per wave were then drawn one by one — 12 k single draws
    // and 3 k failing ones queued on the one word at the end of each leaf kernel, ~0.1 ms of every pass whatever
    // its size (scripts/leaf_wavelog.py: on an 8-way shard of C(32,16) the waves of k_enum_leaves<1> lived 9 %
    // longer per item than on the whole range).  A wave that sees the end of the table tells its siblings.
    constexpr int kRun = 4;
    const int nwaves = (int)gridDim.x * LEAF_WAVES;
    const int k0 = max(1, min(kRun, nitems / (nwaves * 4)));
    const int dyn_base = nwaves * k0;
    auto pack_run = [](int next, int end) { return ((unsigned long long)(unsigned)next << 32) | (unsigned)end; };
    {
        const int first = ((int)blockIdx.x * LEAF_WAVES + wave) * k0;
        if (lane == 0) s_run[wave] = pack_run(min(first, nitems), min(first + k0, nitems));
        if (tid == 0) s_dry = 0;
    }
    __syncthreads();
    auto take = [&](int w) {   // the next item of wave w's run, -1 if it is empty
        int item = -1;
        if (lane == 0) {
            unsigned long long cur = __hip_atomic_load(&s_run[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            while ((unsigned)(cur >> 32) < (unsigned)cur) {
                if (__hip_atomic_compare_exchange_strong(&s_run[w], &cur, cur + (1ULL << 32), __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                    item = (int)(cur >> 32);
                    break;
                }
            }
        }
        return __builtin_amdgcn_readfirstlane(item);
    };
    bool dry = dyn_base >= nitems;   // the table is dealt out
    bool none = false;               // this wave has been told "nothing left" (final: the loop below ends on the first
                                     // such answer, so a later, luckier draw — a sibling's last run arriving — would be lost)
    auto draw = [&]() {
        if (none) return nitems;
        int item = take(wave);
        if (item >= 0) return item;
        if (!dry && __hip_atomic_load(&s_dry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) dry = true;
        if (!dry) {
            constexpr int k = kRun;
            int v = 0, over = 0;
            if (lane == 0) {
                v = atomicAdd(cursor, k);
                // a list far beyond its capacity (a degenerate LP): the caller switches to the dense form
                // whatever else this pass finds, so the waves stop drawing (the load rides with the atomic)
                over = __hip_atomic_load(pd.list_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > pd.list_abort;
            }
            v = __builtin_amdgcn_readfirstlane(v) + dyn_base;
            if (__builtin_amdgcn_readfirstlane(over)) v = nitems;
            if (v < nitems) {
                if (k > 1 && lane == 0)
                    __hip_atomic_store(&s_run[wave], pack_run(v + 1, min(v + k, nitems)), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                return v;
            }
            dry = true;
            if (lane == 0) __hip_atomic_store(&s_dry, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        for (int q = 1; q < LEAF_WAVES; ++q) {
            item = take((wave + q) & (LEAF_WAVES - 1));
#ifdef LP_LEAF_WAVELOG
            if (item >= 0) ++wl_steals;
#endif
            if (item >= 0) return item;
        }
        none = true;
        return nitems;
    };
    double pre[NLOAD];
    NodeMeta pmB;
    int chunkB = 0, childB = 0, roffB = 0, recB = 0;
    auto fetch = [&](int item) {   // issue the loads of item's record (no use of the data here)
        const int4 it = items[item];
        recB = it.x;
        childB = it.y;
        chunkB = it.z;
        roffB = it.w;
        const double* Q = roots + (size_t)it.x * rec_doubles(n, D);
#pragma unroll
        for (int q = 0; q < NLOAD; ++q) {
            const int k = lane + 64 * q;
            pre[q] = (k < rec_cols * PG) ? Q[k] : 0.0;
        }
        pmB = *reinterpret_cast<const NodeMeta*>(Q + (size_t)PG * rec_cols);
    };
    int itemB = draw();
    int itemC = draw();
    if (itemB < nitems) fetch(itemB);
    int buf = 0;
    for (;;) {
        if (itemB >= nitems) break;
#ifdef LP_LEAF_WAVELOG
        if (!wl_items) wl_t1 = __builtin_amdgcn_s_memrealtime();
        ++wl_items;
#endif
        // ---- item B becomes the current item: registers -> LDS slice (odd column stride)
        // (table 1: the item's fields in scalar registers — the bounds of its groups and sub-groups
        // and their cuts to [begin, end) below are then scalar arithmetic)
        auto field = [](int v) { return MODE == 3 ? __builtin_amdgcn_readfirstlane(v) : v; };
        const int chunk = field(chunkB), child = field(childB), roff = field(roffB), rec = recB;
        const NodeMeta pm = pmB;
        double* tab = s_tab[wave * 2 + buf];
#pragma unroll
        for (int q = 0; q < NLOAD; ++q) {
            const int k = lane + 64 * q;
            if (k < rec_cols * PG) tab[(k >> 4) * TS + (k & 15)] = pre[q];
        }
        buf ^= 1;
        itemB = itemC;
        itemC = draw();
        if (itemB < nitems) fetch(itemB);
        if (pm.last_col == kHole) continue;
        const int child_col = FUSED ? (child & 0xFF) : pm.last_col;   // last chosen column of the depth m-6 node
        const int j2_first = (child >> 8) & 0xFF;      // MODE 3: first remaining column of the (first) group
        const int ngroups = child >> 16;               // MODE 3: groups packed into this item
        const int last = child_col;
        const int R = n - 1 - last;                    // selectable columns of the depth m-6 node
        if (R < KD) continue;
        // subsets of this item: [leaf_lo, leaf_hi) inside the node (MODE 0/1) or inside the group (MODE 3)
        const unsigned int L = s_binom[R * (KD + 1) + KD];   // (MODE 0/1)
        // subset table: all 6-subsets of R columns in lexicographic order, 5 bits per index
        // (one L2-resident load; a dependent unranking loop over binomials costs ~2k cycles)
        const unsigned* comb = pd.comb6 + s_off[MODE == 3 ? 0 : R];
        unsigned long long rb = pm.rank_base + (unsigned long long)(FUSED ? roff : 0);
        if (MODE == 3) rb = uniform64(rb);
        const unsigned int leaf_lo = (unsigned int)chunk;
        const unsigned int leaf_hi = (leaf_lo + width < L) ? leaf_lo + width : L;
        double minp0 = pm.minp, maxp0 = pm.maxp;
        unsigned umask = __builtin_amdgcn_readfirstlane(pm.used_mask);
        bool sing0 = false;   // MODE 1: the first child of a paired item turned out singular
        if (FUSED) {
            // ---- the wave pivots on column `child`: lane = (row r, column group g), exactly the
            // arithmetic of the level kernels (first unused row of largest |w|; l = -(w/piv) as w * (1/piv))
            const int r = lane & (PG - 1), g = lane >> 4;
            const bool row_used = (r >= m) || ((umask >> r) & 1u);
            const double* pcol = tab + (child_col - D) * TS;
            const double w = pcol[r];
            double big;
            const int p = __builtin_amdgcn_readfirstlane(pick_pivot_row(w, row_used, lane & ~(PG - 1), big));
            minp0 = fmin(minp0, big);
            maxp0 = fmax(maxp0, big);
            if (!(big > 0.0) || minp0 <= DBL_EPSILON * (double)m * maxp0) {
                // every subset below this node is singular
                unsigned int span = leaf_hi - leaf_lo;
                if (MODE == 3) {
                    span = 0;
                    for (int gi = 0; gi < ngroups; ++gi) span += s_binom[(R - 1 - j2_first - gi) * (KD + 1) + KD - 1];
                    if (ngroups == 1) span = min(span - leaf_lo, width);
                }
                if (lane == 0) cntS += (unsigned int)overlap(rb + leaf_lo, span, begin, end);
                if (MODE == 1 && ((child >> 16) & 1))
                    sing0 = true;   // the item's second child is still to do
                else
                    continue;
            }
            const double inv = 1.0 / pcol[p];
            const bool isp = (r == p);
            const double lx = isp ? inv : -(w * inv);
            umask |= 1u << p;
            // The child's rows are written PERMUTED: the 6 rows still unused (ascending) at positions
            // 0..5, the used ones (ascending) behind them — leaf_verdict<PERM> then reads every row at
            // a compile-time offset.
            // (`below` is recomputed per item — the opaque copy of r keeps it from being hoisted out of the item
            // loop, where it was spilled to scratch and reloaded in front of the row permutation)
            unsigned rr = (unsigned)r;
            asm volatile("" : "+v"(rr));
            const unsigned all = (1u << m) - 1u, below = (1u << rr) - 1u, freem = ~umask & all;
            const int pos = (r >= m) ? r
                            : ((freem >> r) & 1u) ? __builtin_popcount(freem & below)
                                                  : __builtin_popcount(freem) + __builtin_popcount(umask & all & below);
            double* ctab = s_child[wave];
            // The rounds end at the tableau's own width (a wave-uniform branch; six rounds whatever the width cost a
            // 10-column child three rounds of address arithmetic for nothing).  MODE 1: the subsets of a table-0 item
            // are the child's tail, whose first remaining column leaves fewer than kGrandMin selectable ones — they
            // reach only the last kGrandMin columns and the rhs, so only those are written (at their own positions).
            // MODE 3: the item's groups pivot on columns j2_first .. and read the ones behind them.
            // (C(32,16): SQ_INSTS_VALU of table 1's kernel 2.520 -> 2.513 G per pass, none in table 0's, whose rounds
            // beyond the width were skipped by an execz branch already; with the row maximum and the item width the
            // bench step 12.98 -> 12.75 ms and the slowest 8-way shard 2.07 -> 1.96 ms: profiles/enum_leaf_steps.json)
            const int Ru = __builtin_amdgcn_readfirstlane(R);
            const int jlo = MODE == 1 ? max(Ru - kGrandMin, 0) : MODE == 3 ? __builtin_amdgcn_readfirstlane(j2_first) : 0;
#pragma unroll
            for (int q = 0; q < (CHILDCOLS + 3) / 4; ++q) {
                if (jlo + 4 * q > Ru) break;
                const int j = jlo + g + 4 * q;      // child column j = column child+1+j (j = R: rhs)
                if (j <= R && !sing0) {
                    const double* pc = tab + (child_col + 1 + j - D) * TS;
                    ctab[j * TS + pos] = fma(lx, pc[p], isp ? -0.0 : pc[r]);
                }
            }
            tab = ctab;
        } else {
            tab += (last + 1 - D) * TS;              // column q below = column last+1+q
            // (m = 6: the root record, no row used yet — the identity is the permuted order)
        }
        if constexpr (MODE == 3) {
            constexpr int K5 = KD - 1;
            const double minp1 = minp0, maxp1 = maxp0;
            for (int gi = 0; gi < ngroups; ++gi) {
            // ---- second pivot, on column j2 of the (row-permuted) child tableau: positions 0..5 are
            // the unused rows in ascending original order, so "first row of largest |w|" keeps its meaning
            const int j2 = j2_first + gi;
            const int R2 = R - 1 - j2;                 // selectable columns of the depth m-5 node
            const unsigned int L2 = uniform_len(s_binom[R2 * (KD + 1) + K5]);
            const unsigned int lo2 = leaf_lo;          // (0 unless the item is a chunk of one large group)
            const unsigned int hi2 = (lo2 + width < L2) ? lo2 + width : L2;
            const unsigned long long rb2 = rb;
            rb += L2;                                  // next group of a packed item
            // [begin, end) as leaf indices of this group, [wlo, whi) — saturated at 2^32 - 1, far
            // beyond a group's C(21, 5) subsets — so that the cuts below are 32-bit scalar min / max
            const unsigned long long rlo = begin > rb2 ? begin - rb2 : 0ULL, rhi = end > rb2 ? end - rb2 : 0ULL;
            const unsigned int wlo = rlo < 0xFFFFFFFFULL ? (unsigned int)rlo : ~0u;
            const unsigned int whi = rhi < 0xFFFFFFFFULL ? (unsigned int)rhi : ~0u;
            // leaves [a, b) of the group, a < b, cut to the window (b <= a: none inside), and how many are inside
            auto cut = [&](unsigned int& a, unsigned int& b) {
                a = max(a, wlo);
                b = min(b, whi);
            };
            auto inside = [&](unsigned int a, unsigned int b) {
                cut(a, b);
                return b > a ? b - a : 0u;
            };
            if (inside(lo2, hi2) == 0u) continue;
            const int r = lane & (PG - 1), g = lane >> 4;
            const double* pcol = tab + j2 * TS;
            const double w = pcol[r];
            double big;
            const int p2 = __builtin_amdgcn_readfirstlane(pick_pivot_row(w, r >= KD, lane & ~(PG - 1), big));
            const double minp2 = leaf_min(minp1, big), maxp2 = leaf_max(maxp1, big);   // (big: a v_max_f64 result)
            if (!(big > 0.0) || minp2 <= DBL_EPSILON * (double)m * maxp2) {
                if (lane == 0) cntS += inside(lo2, hi2);
                continue;
            }
            const double inv = 1.0 / pcol[p2];
            const bool isp = (r == p2);
            const double lx = isp ? inv : -(w * inv);
            // rows of the grandchild: the 5 unused ones at 0..4, the new pivot row at 5, the rest stay
            const int pos = (r < p2) ? r : (r == p2) ? K5 : (r < KD) ? r - 1 : r;
            double* gtab = s_grand[wave];
            const int R2u = __builtin_amdgcn_readfirstlane(R2);
            const unsigned* comb5 = pd.comb5 + uniform_off(s_off[R2]);
            // The 5-column loop's bounds, known before the sub-groups run: the sub-groups are the first remaining
            // columns j3 that leave k = R2-1 .. kGreatMin selectable ones, sum of C(k, 4) = C(R2, 5) - C(kGreatMin, 5)
            // subsets (if the sub-group loop below ends early, at off3 >= hi2, this is >= hi2 as well: no tail either way).
            unsigned int tail_lo = lo2;                // the leaves in front of it went to sub-groups
            if (R2 >= kGreatMin) tail_lo = max(lo2, L2 - uniform_len(s_binom[kGreatMin * (KD + 1) + K5]));
            unsigned int tl = tail_lo, th = hi2;       // ... and cut to [begin, end)
            cut(tl, th);
            // The first pass's table word is issued here: the copy rounds and the sub-groups hide its round trip.
            // (Clamped index: a lane past the loop's end reads the group's last word and never uses it.)
            unsigned pk5 = comb_word(comb5, min(tl + (unsigned)lane, hi2 - 1u));
#pragma unroll
            for (int q = 0; q < (NMX + KD + 3) / 4; ++q) {
                if (4 * q > R2u) break;
                const int j = g + 4 * q;        // grandchild column j = child column j2+1+j (j = R2: rhs)
                if (j <= R2) {
                    const double* pc = tab + (j2 + 1 + j) * TS;
                    gtab[j * TS + pos] = fma(lx, pc[p2], isp ? -0.0 : pc[r]);
                }
            }
            const int U5[K5] = {0, 1, 2, 3, 4};        // unused by leaf_verdict<PERM>
            constexpr int K4 = KD - 2;
            double* ggtab = s_tab[wave * 2 + buf];  // (the next item's slice: written at the top of the next iteration)
            unsigned int off3 = 0;                  // first leaf of sub-group j3 inside the group
            for (int j3 = 0; R2 - 1 - j3 >= kGreatMin && off3 < hi2; ++j3) {
                const int R3 = R2 - 1 - j3;         // selectable columns of the depth m-4 node
                const unsigned int L3 = uniform_len(s_binom[R3 * (KD + 1) + K4]);
                const unsigned int a3 = off3 > lo2 ? off3 : lo2, b3 = off3 + L3 < hi2 ? off3 + L3 : hi2;
                const unsigned int base3 = off3;
                off3 += L3;
                if (a3 >= b3 || inside(a3, b3) == 0u) continue;
                // ---- third pivot, on column j3 of the grandchild tableau (unused rows at positions 0..4, ascending)
                const double* pcol3 = gtab + j3 * TS;
                const double w3 = pcol3[r];
                double big3;
                const int p3 = __builtin_amdgcn_readfirstlane(pick_pivot_row(w3, r >= K5, lane & ~(PG - 1), big3));
                const double minp3 = leaf_min(minp2, big3), maxp3 = leaf_max(maxp2, big3);
                if (!(big3 > 0.0) || minp3 <= DBL_EPSILON * (double)m * maxp3) {
                    if (lane == 0) cntS += inside(a3, b3);
                    continue;
                }
                const double inv3 = 1.0 / pcol3[p3];
                const bool isp3 = (r == p3);
                const double lx3 = isp3 ? inv3 : -(w3 * inv3);
                // rows: the 4 unused ones at 0..3, the new pivot row at 4, the rest stay
                const int pos3 = (r < p3) ? r : (r == p3) ? K4 : (r < K5) ? r - 1 : r;
                const int R3u = __builtin_amdgcn_readfirstlane(R3);
                // the sub-group's table (words relative to the group's leaf 0), its loop bounds cut to
                // [begin, end), and the first pass's word, issued in front of the copy rounds
                const unsigned* comb4 = pd.comb4 + uniform_off(s_off4[R3]) - uniform_off(base3);
                unsigned int a3w = a3, b3w = b3;
                cut(a3w, b3w);
                unsigned pk4 = comb_word(comb4, min(a3w + (unsigned)lane, b3 - 1u));
#pragma unroll
                for (int q = 0; q < (NMX + KD + 2) / 4; ++q) {
                    if (4 * q > R3u) break;
                    const int j = g + 4 * q;        // column j = grandchild column j3+1+j (j = R3: rhs)
                    if (j <= R3) {
                        const double* pc = gtab + (j3 + 1 + j) * TS;
                        ggtab[j * TS + pos3] = fma(lx3, pc[p3], isp3 ? -0.0 : pc[r]);
                    }
                }
                const int U4[K4] = {0, 1, 2, 3};    // unused by leaf_verdict<PERM>
                for (unsigned int leaf = a3w + lane; leaf < b3w; leaf += 64) {
                    const unsigned long long rank = rb2 + leaf;
                    int c4[K4];
                    // this pass's word was loaded a pass ago; the next pass's is in flight during the verdicts
                    // (index clamped to the sub-group's last leaf: no read past its table, no branch)
                    const unsigned pk = pk4;
                    pk4 = comb_word(comb4, min(leaf + 64u, b3 - 1u));
#pragma unroll
                    for (int t = 0; t < K4; ++t) c4[t] = (int)((pk >> (5 * t)) & 31u);
                    const int verdict = leaf_verdict<K4, TS, true, false, !EXACT, true>(ggtab, c4, R3, U4, 0u, minp3, maxp3, m, nullptr, &viol, s_rows4);
                    if (verdict == 2) {
                        ++cntS;
                    } else if (verdict == 1) {
                        ++cntI;
                    } else {
                        ++cntF;
                        const unsigned long long at = atomicAdd(pd.list_count, 1ULL);
                        if (at < pd.list_cap) {
                            pd.list[at] = rank;
                            pd.list_rec[at] = rec;
                        }
                    }
                }
            }
            for (unsigned int leaf = tl + lane; leaf < th; leaf += 64) {
                const unsigned long long rank = rb2 + leaf;
                int c[K5];
                const unsigned pk = pk5;   // (as the sub-groups' loop: one pass ahead, clamped to the group's last leaf)
                pk5 = comb_word(comb5, min(leaf + 64u, hi2 - 1u));
#pragma unroll
                for (int t = 0; t < K5; ++t) c[t] = (int)((pk >> (5 * t)) & 31u);
                const int verdict = leaf_verdict<K5, TS, true, false, !EXACT, true>(gtab, c, R2, U5, 0u, minp2, maxp2, m, nullptr, &viol, s_rows);
                if (verdict == 2) {
                    ++cntS;
                } else if (verdict == 1) {
                    ++cntI;
                } else {
                    ++cntF;
                    const unsigned long long at = atomicAdd(pd.list_count, 1ULL);
                    if (at < pd.list_cap) {
                        pd.list[at] = rank;
                        pd.list_rec[at] = rec;
                    }
                }
            }
            }
        } else if constexpr (MODE == 1) {
            // ---- table 0 item: the tail [leaf_lo, L) of child `child_col` and, if flagged, of the next
            // child too (pivoted from the same record): the lanes are filled from both tails
            const bool pair = (child >> 16) & 1;
            const double* par = s_tab[wave * 2 + (buf ^ 1)];   // the record's slice (tab now points at the child)
            unsigned int T0 = sing0 ? 0u : L - leaf_lo, T1 = 0, lo1 = 0;
            unsigned long long rb1 = rb + L;
            double minq = pm.minp, maxq = pm.maxp;
            const double* tab1 = tab;
            int R1 = R - 1;
            if (pair) {
                for (int j2 = 0; R1 - 1 - j2 >= kGrandMin; ++j2) lo1 += s_binom[(R1 - 1 - j2) * (KD + 1) + KD - 1];
                const unsigned int L1 = s_binom[R1 * (KD + 1) + KD];
                T1 = L1 - lo1;
                // second pivot, on column child_col + 1 of the record
                const int r = lane & (PG - 1), g = lane >> 4;
                unsigned um1 = __builtin_amdgcn_readfirstlane(pm.used_mask);
                const bool row_used = (r >= m) || ((um1 >> r) & 1u);
                const double* pcol = par + (child_col + 1 - D) * TS;
                const double w = pcol[r];
                double big;
                const int p = __builtin_amdgcn_readfirstlane(pick_pivot_row(w, row_used, lane & ~(PG - 1), big));
                minq = fmin(minq, big);
                maxq = fmax(maxq, big);
                if (!(big > 0.0) || minq <= DBL_EPSILON * (double)m * maxq) {
                    if (lane == 0) cntS += (unsigned int)overlap(rb1 + lo1, T1, begin, end);
                    T1 = 0;   // every subset below the second child is singular
                } else {
                    const double inv = 1.0 / pcol[p];
                    const bool isp = (r == p);
                    const double lx = isp ? inv : -(w * inv);
                    um1 |= 1u << p;
                    unsigned rr = (unsigned)r;
                    asm volatile("" : "+v"(rr));
                    const unsigned all = (1u << m) - 1u, below = (1u << rr) - 1u, freem = ~um1 & all;
                    const int pos = (r >= m) ? r
                                    : ((freem >> r) & 1u) ? __builtin_popcount(freem & below)
                                                          : __builtin_popcount(freem) + __builtin_popcount(um1 & all & below);
                    int wv = wave;   // (opaque copy: the slice address is recomputed here, not kept live — and spilled — across items)
                    asm volatile("" : "+v"(wv));
                    double* ctab1 = s_child2[wv];
                    const int R1u = __builtin_amdgcn_readfirstlane(R1), jlo1 = max(R1u - kGrandMin, 0);   // (as the first child's)
#pragma unroll
                    for (int q = 0; q < (CHILDCOLS + 3) / 4; ++q) {
                        if (jlo1 + 4 * q > R1u) break;
                        const int j = jlo1 + g + 4 * q;   // column j of the second child = record column child_col+2+j
                        if (j <= R1) {
                            const double* pc = par + (child_col + 2 + j - D) * TS;
                            ctab1[j * TS + pos] = fma(lx, pc[p], isp ? -0.0 : pc[r]);
                        }
                    }
                    tab1 = ctab1;
                }
            }
            const unsigned* comb1 = pd.comb6 + s_off[R1 >= KD ? R1 : KD];
            const int U[KD] = {0, 1, 2, 3, 4, 5};        // unused by leaf_verdict<PERM>
            for (unsigned int gidx = lane; gidx < T0 + T1; gidx += 64) {
                const bool second = gidx >= T0;
                const unsigned int leaf = second ? lo1 + (gidx - T0) : leaf_lo + gidx;
                const unsigned long long rank = (second ? rb1 : rb) + leaf;
                if (rank < begin || rank >= end) continue;
                int c[KD];
                const unsigned pk = (second ? comb1 : comb)[leaf];
#pragma unroll
                for (int t = 0; t < KD; ++t) c[t] = (int)((pk >> (5 * t)) & 31u);
                const int verdict = leaf_verdict<KD, TS, true, false, !EXACT, true>(second ? tab1 : tab, c, second ? R1 : R, U, 0u,
                                                                              second ? minq : minp0, second ? maxq : maxp0, m,
                                                                              nullptr, &viol, s_rows);
                if (verdict == 2) {
                    ++cntS;
                } else if (verdict == 1) {
                    ++cntI;
                } else {
                    ++cntF;
                    const unsigned long long at = atomicAdd(pd.list_count, 1ULL);
                    if (at < pd.list_cap) {
                        pd.list[at] = rank;
                        pd.list_rec[at] = rec;
                    }
                }
            }
        } else {
        const int U[KD] = {0, 1, 2, 3, 4, 5};        // unused by leaf_verdict<PERM>
        // (m = 6: bounds cut to [begin, end) and the table word one pass ahead, as k_enum_leaves<3>'s loops)
        const unsigned* comb0 = pd.comb6 + uniform_off(s_off[R]);
        unsigned int l0 = leaf_lo, l1 = leaf_hi;
        clamp_to_window(rb, l0, l1, begin, end);
        unsigned pk6 = comb_word(comb0, min(l0 + (unsigned)lane, leaf_hi - 1u));
        for (unsigned int leaf = l0 + lane; leaf < l1; leaf += 64) {
            const unsigned long long rank = rb + leaf;
            int c[KD];
            const unsigned pk = pk6;
            pk6 = comb_word(comb0, min(leaf + 64u, leaf_hi - 1u));
#pragma unroll
            for (int t = 0; t < KD; ++t) c[t] = (int)((pk >> (5 * t)) & 31u);
            const int verdict = leaf_verdict<KD, TS, true, false, !EXACT, true>(tab, c, R, U, umask, minp0, maxp0, m, nullptr, &viol, s_rows);
            if (verdict == 2) {
                ++cntS;
            } else if (verdict == 1) {
                ++cntI;
            } else {
                ++cntF;
                const unsigned long long at = atomicAdd(pd.list_count, 1ULL);
                if (at < pd.list_cap) {
            pd.list[at] = rank;
            pd.list_rec[at] = rec;
        }
            }
        }
        }
    }
#ifdef LP_LEAF_WAVELOG
    wavelog_put(MODE, wl_t0, wl_t1, wl_items, wl_steals);
#endif
    if (cntF) atomicAdd(&s_cnt[0], (unsigned long long)cntF);
    if (cntI) atomicAdd(&s_cnt[1], (unsigned long long)cntI);
    if (cntS) atomicAdd(&s_cnt[2], (unsigned long long)cntS);
    if (!EXACT && viol) atomicOr(&d.result->range_flag, 1ULL);
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(&d.result->counts[tid], s_cnt[tid]);
}

// The tails: for every depth m-7 record, the 7-subsets inside its last T' = min(R, T) selectable columns (T = THIN_TAIL) —
// the last C(T',7) subsets of the record in rank order, in the lexicographic order of those T' columns (s_comb).
// Lanes are packed densely: a wave takes a batch of 64 consecutive records, one lane reads each record's metadata
// (the next batch's is in flight meanwhile), the records that have subsets inside [begin, end) are compacted into the
// wave's LDS list with the prefix sums of their subset counts, and passes of 64 consecutive subsets run over that
// list — a record with one subset costs one lane, not eight.  The columns a pass needs (last T' columns + rhs: one
// contiguous run of 128-byte columns per record) are loaded coalesced one pass ahead, and written to the wave's LDS
// slots with the rows permuted by the record's used_mask (the 7 unused rows first, ascending; as the child pivot's
// write in k_enum_leaves), so that the lanes run leaf_verdict<PERM>: rows of steps 0 and 1 chosen before loading, no
// rotation selects, phase 2 from LDS.  A pass ends after 64 subsets or kTailSlots records, whichever comes first.
// (Row offsets of the other five rows: leaf_verdict's computed branch, ~25 integer instructions per subset of
// ~900; a 49-entry table of 64-bit words would save ~15 of them for two more LDS reads.)
// Registers: seven columns per lane are 49 + 7 doubles of matrix and 30 of stored pivot rows; with the staged columns
// the kernel needs 254 VGPRs (2 waves per SIMD).  Held to the leaf kernels' 168 it spills 127-364 registers, and the
// scratch reloads, which share the loads' in-order counter, serialise every pass: C(32,16) 23-35 ms against 13.
// kTailSlots: passes made of one-subset records fill only that many lanes; 4 slots instead of 8 cost 8 % of the pass
// at 8 columns (15.5 against 14.4 ms with the kernel beside the leaf kernels), 16 would not fit the registers.
constexpr int kTailSlots = 8;                               // records staged per pass and wave
// doubles per staged record of T + 1 columns: odd, so that lanes reading the same row and column of different records
// hit different banks
constexpr int tail_slot(int T) { return ((T + 1) * TS) | 1; }
constexpr int tail_iter(int T) { return (T + 1 + 3) / 4; }  // columns per 16-lane group and staged record (4 groups per wave)
__host__ __device__ constexpr int tail_count(int tp) { return tp == 7 ? 1 : tp == 8 ? 8 : 36; }     // C(tp, 7), tp <= 9
__host__ __device__ constexpr int tail_comb_off(int tp) { return tp == 7 ? 0 : tp == 8 ? 1 : 9; }   // sum of the counts below tp
constexpr int tail_comb(int T) { return tail_comb_off(T) + tail_count(T); }   // 7-subsets of 7 .. T columns
// s_waitcnt vmcnt(0) in the gfx9 encoding of the instruction's immediate: vmcnt = bits 3:0 and 15:14 (all zero),
// expcnt = bits 6:4 (7: not waited for), lgkmcnt = bits 11:8 (15: not waited for)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "k_enum_thin: kWaitVm0 is the gfx9 encoding of s_waitcnt"
#endif
constexpr int kWaitVm0 = 0x0F70;
struct alignas(16) TailRec {
    unsigned long long rank0;   // rank of the record's first tail subset
    unsigned used;              // rows used by the prefix
    unsigned src;               // lane that holds the record's metadata (= record index inside the batch) | T' << 8
};

template <bool EXACT, int T>
__global__ __launch_bounds__(LEAF_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_enum_thin(EnumDev d, PrefixDev pd,
                                                             const double* __restrict__ roots,
                                                             int root_level, int root_cap,
                                                             unsigned long long begin,
                                                             unsigned long long end) {
    static_assert(T == 8 || T == 9, "k_enum_thin: subset table, counts and LDS slots are written for 8 and 9 columns");
    constexpr int KD = 7, kTailSlot = tail_slot(T), kTailIter = tail_iter(T), kTailComb = tail_comb(T);
    __shared__ __attribute__((aligned(16))) double s_slot[LEAF_WAVES][kTailSlots * kTailSlot];
    __shared__ TailRec s_rec[LEAF_WAVES][64];   // the batch's records that have tail subsets in range, compacted
    __shared__ int s_pre[LEAF_WAVES][65];       // exclusive prefix sums of their subset counts (+ the total)
    __shared__ unsigned int s_comb[kTailComb];  // 7-subsets of T' columns in lexicographic order, 4 bits per index
    __shared__ unsigned int s_b7[NMX + KD + 2]; // C(r, 7)
    __shared__ unsigned long long s_cnt[3];
    const int m = d.m, n = d.n, D = m - KD;
    const int nrec = min(pd.level_counts[root_level], root_cap);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef LP_LEAF_WAVELOG
    const unsigned long long wl_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    if (tid < 3) s_cnt[tid] = 0ULL;
    if (tid < NMX + KD + 2) s_b7[tid] = (unsigned int)d.binom[tid * kBinomK + KD];
    if (tid < kTailComb) {
        const int tp = tid < tail_comb_off(8) ? 7 : tid < tail_comb_off(9) ? 8 : 9;
        unsigned long long j = (unsigned long long)(tid - tail_comb_off(tp));
        unsigned pk = 0;
        int x = 0;
        for (int t = 0; t < KD; ++t) {
            for (; x < tp; ++x) {   // subsets whose t-th column is x: C(tp - 1 - x, 6 - t)
                const unsigned long long cx = binom(d, tp - 1 - x, KD - 1 - t);
                if (j < cx) break;
                j -= cx;
            }
            pk |= (unsigned)x << (4 * t);
            ++x;
        }
        s_comb[tid] = pk;
    }
    __syncthreads();
    unsigned int cnt[3] = {0u, 0u, 0u};
    unsigned int viol = 0;
    double* const slots = s_slot[wave];
    TailRec* const recs = s_rec[wave];
    int* const pre = s_pre[wave];
    const int nbatch = (nrec + 63) >> 6;
    const int nw = (int)gridDim.x * LEAF_WAVES;
    const size_t recd = rec_doubles(n, D);
    const int row = lane & (PG - 1), cg = lane >> 4;   // staging: lane = (row, one of 4 columns)
    const unsigned all = (1u << m) - 1u, below = (1u << row) - 1u;
    // one lane per record of a batch; the metadata of the wave's next batch is loaded a batch ahead
    int lastN = kHole;
    unsigned usedN = 0;
    unsigned long long rbN = 0ULL;
    double minN = 0.0, maxN = 0.0;
    auto meta = [&](int batch) {
        const int rec = batch * 64 + lane;
        lastN = kHole;
        if (batch < nbatch && rec < nrec) {
            const NodeMeta* pm = reinterpret_cast<const NodeMeta*>(roots + (size_t)rec * recd + (size_t)PG * (n - D + 1));
            lastN = pm->last_col;
            usedN = pm->used_mask;
            rbN = pm->rank_base;
            minN = pm->minp;
            maxN = pm->maxp;
        }
    };
    double stage[kTailSlots * kTailIter] = {};   // a pass's columns in flight
    int batch = (int)blockIdx.x * LEAF_WAVES + wave;
    meta(batch);
    for (; batch < nbatch; batch += nw) {
        const int last = lastN;
        const unsigned used = usedN;
        const unsigned long long rb = rbN;
        const double minp_l = minN, maxp_l = maxN;
        meta(batch + nw);
        const int recbase = batch * 64;
        // ---- the batch's work list: records with tail subsets in range, prefix sums of their counts
        const int R = n - 1 - last, Tp = R < T ? R : T;
        int c7 = 0;
        unsigned long long rank0 = 0ULL;
        if (last != kHole && R >= KD) {
            c7 = tail_count(Tp);
            rank0 = rb + (unsigned long long)(s_b7[R] - (unsigned int)c7);   // the tail subsets are the record's last ones
            if (overlap(rank0, (unsigned long long)c7, begin, end) == 0ULL) c7 = 0;
        }
        const unsigned long long nz = __ballot(c7 > 0);
        const int nk = __popcll(nz);
        if (nk == 0) continue;
        const int k = __popcll(nz & ((1ULL << lane) - 1ULL));
        int incl = c7;   // inclusive wave scan
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (c7 > 0) {
            pre[k] = incl - c7;
            TailRec tr;
            tr.rank0 = rank0;
            tr.used = used;
            tr.src = (unsigned)lane | ((unsigned)Tp << 8);
            recs[k] = tr;
        }
        if (lane == 63) pre[nk] = incl;
        const int total = __shfl(incl, 63, 64);
        // a pass: subsets [w0, wend) of the list, inside records k0 .. k0 + nslot - 1 (slot = record - k0)
        auto plan = [&](int k0, int w0, int& nslot, int& wend) {
            const int k1 = min(k0 + kTailSlots, nk);
            wend = __builtin_amdgcn_readfirstlane(min(w0 + 64, pre[k1]));
            const bool starts = lane < k1 - k0 && pre[min(k0 + lane, nk)] < wend;
            nslot = __popcll(__ballot(starts));
        };
        // Staging: the 16-lane group cg of a wave takes columns cg, cg + 4, cg + 8 of every slot (lane = row), so a
        // slot costs one address and kTailIter loads / LDS writes at immediate offsets.  The slot's record is
        // wave-uniform: its fields go through scalar registers.
        auto issue = [&](int k0, int nslot) {   // loads of a pass's columns (no use of the data here)
#pragma unroll
            for (int s = 0; s < kTailSlots; ++s) {
                if (s < nslot) {
                    const unsigned srcw = __builtin_amdgcn_readfirstlane(recs[k0 + s].src);
                    const int tp = (int)(srcw >> 8);
                    // column cc of the slot = the record's column n - tp + cc (cc = tp: the rhs)
                    const double* p = roots + (size_t)(recbase + (int)(srcw & 0xFFu)) * recd + (size_t)(n - tp - D) * PG + lane;
                    // (a column past the rhs is replaced by the group's first one and never written to LDS: the load
                    // itself stays unconditional, so that no select waits for its data here)
#pragma unroll
                    for (int i = 0; i < kTailIter; ++i) stage[s * kTailIter + i] = p[(cg + 4 * i <= tp) ? 4 * i * PG : 0];
                }
            }
        };
        auto commit = [&](int k0, int nslot) {  // registers -> LDS slots, rows permuted: unused rows first
#pragma unroll
            for (int s = 0; s < kTailSlots; ++s) {
                if (s < nslot) {
                    const int tp = (int)(__builtin_amdgcn_readfirstlane(recs[k0 + s].src) >> 8);
                    const unsigned usedw = __builtin_amdgcn_readfirstlane(recs[k0 + s].used) & all;
                    const unsigned freem = ~usedw & all;
                    const int pos = (row >= m) ? row
                                    : ((freem >> row) & 1u) ? __builtin_popcount(freem & below)
                                                            : __builtin_popcount(freem) + __builtin_popcount(usedw & below);
                    double* q = slots + s * kTailSlot + cg * TS + pos;
#pragma unroll
                    for (int i = 0; i < kTailIter; ++i)
                        if (cg + 4 * i <= tp) q[4 * i * TS] = stage[s * kTailIter + i];
                }
            }
        };
        int k0 = 0, w0 = 0, nslot, wend;
        plan(k0, w0, nslot, wend);
        issue(k0, nslot);
        for (;;) {
            commit(k0, nslot);
            // Every staged load has landed by now (the slots just written were the last ones issued), and the
            // explicit wait tells the compiler so: without it the generated code guards the reuse of each staging
            // register in the next pass's loads with a wait of its own — the counter is in order, so slot s + 1's
            // loads then wait for slot s's, one HBM round trip per staged record.
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_waitcnt(kWaitVm0);
            // (The next batch's metadata loads are older than this pass's staged loads, which the commit above has
            // waited for already: the counter is in order, so this wait costs them nothing.)
            // the next pass: its first record is the one this pass ends in, unless that one is finished
            const int kn = k0 + nslot - (pre[k0 + nslot] == wend ? 0 : 1);
            const bool more = wend < total;
            int nslotN = 0, wendN = 0;
            if (more) {
                plan(kn, wend, nslotN, wendN);
                issue(kn, nslotN);
            }
            // ---- one subset per lane
            const int w = w0 + lane;
            int s = 0;
            for (int q = 1; q < nslot; ++q) s += (pre[k0 + q] <= w) ? 1 : 0;
            const TailRec tr = recs[k0 + s];
            const int src = (int)(tr.src & 0xFFu), tp = (int)(tr.src >> 8);
            const double minp0 = __shfl(minp_l, src, 64), maxp0 = __shfl(maxp_l, src, 64);
            const int j = w - pre[k0 + s];
            int verdict = -1;
            unsigned long long rank = 0ULL;
            if (w < wend) {
                rank = tr.rank0 + (unsigned long long)j;
                if (rank >= begin && rank < end) {
                    const unsigned pk = s_comb[tail_comb_off(tp) + j];
                    int c[KD];
#pragma unroll
                    for (int t = 0; t < KD; ++t) c[t] = (int)((pk >> (4 * t)) & 15u);
                    const int U[KD] = {0, 1, 2, 3, 4, 5, 6};   // unused by leaf_verdict<PERM>
                    verdict = leaf_verdict<KD, TS, true, false, !EXACT, false>(slots + s * kTailSlot, c, tp, U, 0u, minp0, maxp0, m,
                                                                               nullptr, &viol);
                }
            }
            if (verdict == 0) {
                const unsigned long long at = atomicAdd(pd.list_count, 1ULL);
                if (at < pd.list_cap) {
                    pd.list[at] = rank;
                    pd.list_rec[at] = recbase + src;
                }
            }
            cnt[0] += verdict == 0;
            cnt[1] += verdict == 1;
            cnt[2] += verdict == 2;
            if (!more) break;
            k0 = kn;
            w0 = wend;
            nslot = nslotN;
            wend = wendN;
        }
    }
#ifdef LP_LEAF_WAVELOG
    wavelog_put(7, wl_t0, wl_t0, 0, 0);
#endif
    // counts: wave reduction, one LDS atomic per wave and verdict
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        unsigned int c = cnt[v];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if ((tid & 63) == 0 && c) atomicAdd(&s_cnt[v], (unsigned long long)c);
    }
    if (!EXACT && viol) atomicOr(&d.result->range_flag, 1ULL);
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(&d.result->counts[tid], s_cnt[tid]);
}

// The NARROW depth m-7 nodes finished from their PARENTS' records.  A depth m-7 node with at most T = THIN_TAIL
// selectable columns (last chosen column a >= n-1-T) holds 1, 8 or 36 subsets and no leaf item: as a stored record
// it is (R+1)*128 + 64 bytes written by the last level, read once by k_enum_thin and once by the item builder, and
// such records are three quarters of the level of C(32,16) for 2.7 % of its subsets.  Here they are never stored: the
// last level stops at column n-1-T (k_enum_expand_staged: stop), and this kernel takes the depth m-8 records, which
// stay intact in the other level buffer.  k_enum_thin's structure: a wave takes batches of 64 parents, one lane reads
// each parent's metadata (the next batch's in flight); the narrow children (parent, a), a = max(last+1, n-1-T) ..
// n-8, whose rank interval meets [begin, end) are compacted into the wave's LDS list (up to three per lane: they are
// the LAST C(n-a, 8) subsets of the parent, 36 | 8 | 1) with the prefix sums of their subset counts, and passes of 64
// consecutive subsets run over at most kTailSlots children.  One 16-lane group per child (lane = row, four children
// at a time, two rounds per pass) loads the parent's columns a .. n-1 and the rhs into registers one pass ahead —
// eleven loads of 128 bytes per child — and pivots on column a with the level kernel's arithmetic, operand for operand:
// pick_pivot_row over the rows the parent left unused, plain division, fma(lx, L[c][p], isp ? -0.0 : L[c][row]), the
// pivot row's entry L[c][p] broadcast inside the group (bcast16).  The result goes to the child's LDS slot with the
// rows permuted by used | 1 << p, unused rows first, exactly what k_enum_thin stages from a stored record, and the
// lanes run leaf_verdict<PERM> with the child's min / max |pivot|, which row 0 of the group leaves in LDS.  A child
// the level kernel would have pruned (no pivot, or min <= eps * m * max) has max = -1 there: its lanes inside
// [begin, end) count as singular — together the overlap the level kernel adds for a hole.
// Feasible subsets are listed with record -1 (there is no depth m-7 record: k_enum_eval_records leaves them to
// k_enum_eval_list, which scores them from scratch, same bits).
// A child is loaded by itself; loading a parent once for its three children would save the 8- and 1-subset children's
// loads (half of this kernel's 0.3 GB, out of L2 mostly) for a second kind of slot.
// (A first form staged the raw columns in the slot, lane = (row, one of four columns) as k_enum_thin, and all four
// groups pivoted every slot in place: ~100 instructions per child and 14 spilled registers, 1.56 ms by itself for
// the 16.2 M subsets of C(32,16) against this form's time in lp_enum_launch_parent_tails.)
struct alignas(16) ParentTailRec {
    unsigned long long rank0;   // rank of the child's first subset
    unsigned used;              // rows used by the parent's prefix
    unsigned src;               // lane that holds the parent's metadata (= parent index inside the batch) | T' << 8
};

template <bool EXACT, int T>
__global__ __launch_bounds__(LEAF_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_enum_parent_tails(EnumDev d, PrefixDev pd,
                                                             const double* __restrict__ parents,
                                                             int parent_level, int parent_cap,
                                                             unsigned long long begin,
                                                             unsigned long long end) {
    static_assert(T == 9, "k_enum_parent_tails: three children per parent, 36 | 8 | 1 subsets");
    constexpr int KD = 7, kSlot = tail_slot(T), kCols = T + 2, kRounds = kTailSlots / 4, kTailComb = tail_comb(T), kKids = T - KD + 1;
    static_assert(kTailSlots % 4 == 0, "four children per round");
    __shared__ __attribute__((aligned(16))) double s_slot[LEAF_WAVES][kTailSlots * kSlot];
    __shared__ ParentTailRec s_rec[LEAF_WAVES][64 * kKids];   // the batch's narrow children in range, compacted
    __shared__ int s_pre[LEAF_WAVES][64 * kKids + 1];         // exclusive prefix sums of their subset counts (+ the total)
    __shared__ double s_mm[LEAF_WAVES][kTailSlots][2];        // min / max |pivot| of the staged children (max = -1: pruned)
    __shared__ double s_par[LEAF_WAVES][64][2];               // ... of the batch's parents (by lane)
    __shared__ unsigned int s_comb[kTailComb];  // 7-subsets of T' columns in lexicographic order, 4 bits per index
    __shared__ unsigned int s_b8[NMX + KD + 3]; // C(r, 8)
    __shared__ unsigned long long s_cnt[3];
    const int m = d.m, n = d.n, P = m - KD - 1;   // depth of the parents
    const int nrec = min(pd.level_counts[parent_level], parent_cap);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 3) s_cnt[tid] = 0ULL;
    if (tid < NMX + KD + 3) s_b8[tid] = (unsigned int)d.binom[tid * kBinomK + KD + 1];
    if (tid < kTailComb) {
        const int tp = tid < tail_comb_off(8) ? 7 : tid < tail_comb_off(9) ? 8 : 9;
        unsigned long long j = (unsigned long long)(tid - tail_comb_off(tp));
        unsigned pk = 0;
        int x = 0;
        for (int t = 0; t < KD; ++t) {
            for (; x < tp; ++x) {   // subsets whose t-th column is x: C(tp - 1 - x, 6 - t)
                const unsigned long long cx = binom(d, tp - 1 - x, KD - 1 - t);
                if (j < cx) break;
                j -= cx;
            }
            pk |= (unsigned)x << (4 * t);
            ++x;
        }
        s_comb[tid] = pk;
    }
    __syncthreads();
    unsigned int cnt[3] = {0u, 0u, 0u};
    unsigned int viol = 0;
    double* const slots = s_slot[wave];
    ParentTailRec* const recs = s_rec[wave];
    int* const pre = s_pre[wave];
    const int nbatch = (nrec + 63) >> 6;
    const int nw = (int)gridDim.x * LEAF_WAVES;
    const size_t recd = rec_doubles(n, P);
    const int row = lane & (PG - 1), cg = lane >> 4, gbase = lane & ~(PG - 1);   // pivots: lane = (row, one of 4 children)
    const unsigned all = (1u << m) - 1u, below = (1u << row) - 1u;
    const double epsm = DBL_EPSILON * (double)m;
    int lastN = kHole;
    unsigned usedN = 0;
    unsigned long long rbN = 0ULL;
    double minN = 0.0, maxN = 0.0;
    auto meta = [&](int batch) {
        const int rec = batch * 64 + lane;
        lastN = kHole;
        if (batch < nbatch && rec < nrec) {
            const NodeMeta* pm = reinterpret_cast<const NodeMeta*>(parents + (size_t)rec * recd + (size_t)PG * (n - P + 1));
            lastN = pm->last_col;
            usedN = pm->used_mask;
            rbN = pm->rank_base;
            minN = pm->minp;
            maxN = pm->maxp;
        }
    };
    double stage[kRounds * kCols] = {};   // a pass's columns in flight: kCols per child, this group's child of each round
    int batch = (int)blockIdx.x * LEAF_WAVES + wave;
    meta(batch);
    for (; batch < nbatch; batch += nw) {
        const int last = lastN;
        const unsigned used = usedN;
        const unsigned long long rb = rbN;
        s_par[wave][lane][0] = minN;
        s_par[wave][lane][1] = maxN;
        meta(batch + nw);
        const int recbase = batch * 64;
        // ---- the batch's work list: this parent's narrow children in range (ascending a = rank order)
        const int Rp = n - 1 - last;   // the parent's selectable columns: C(Rp, 8) subsets, the narrow children's last
        int ne = 0, c7 = 0;
        unsigned kept = 0;             // bit ci: child a = n - 1 - (T - ci) is kept
        const unsigned long long endp = rb + (unsigned long long)s_b8[(last != kHole && Rp >= KD + 1) ? Rp : 0];
        if (last != kHole && Rp >= KD + 1) {
#pragma unroll
            for (int ci = 0; ci < kKids; ++ci) {
                const int tp = T - ci;
                const unsigned long long rank0 = endp - (unsigned long long)(tail_comb_off(tp) + tail_count(tp));   // C(tp + 1, 8)
                if (n - 1 - tp > last && overlap(rank0, (unsigned long long)tail_count(tp), begin, end) != 0ULL) {
                    kept |= 1u << ci;
                    ++ne;
                    c7 += tail_count(tp);
                }
            }
        }
        int inclE = ne, incl = c7;   // inclusive wave scans: entries, subsets
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int oe = __shfl_up(inclE, off, 64), o = __shfl_up(incl, off, 64);
            if (lane >= off) {
                inclE += oe;
                incl += o;
            }
        }
        const int nk = __shfl(inclE, 63, 64);
        if (nk == 0) continue;
        {
            int k = inclE - ne, at = incl - c7;
#pragma unroll
            for (int ci = 0; ci < kKids; ++ci) {
                if ((kept >> ci) & 1u) {
                    const int tp = T - ci;
                    pre[k] = at;
                    ParentTailRec tr;
                    tr.rank0 = endp - (unsigned long long)(tail_comb_off(tp) + tail_count(tp));
                    tr.used = used;
                    tr.src = (unsigned)lane | ((unsigned)tp << 8);
                    recs[k] = tr;
                    ++k;
                    at += tail_count(tp);
                }
            }
        }
        if (lane == 63) pre[nk] = incl;
        const int total = __shfl(incl, 63, 64);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // a pass: subsets [w0, wend) of the list, inside children k0 .. k0 + nslot - 1 (slot = child - k0)
        auto plan = [&](int k0, int w0, int& nslot, int& wend) {
            const int k1 = min(k0 + kTailSlots, nk);
            wend = __builtin_amdgcn_readfirstlane(min(w0 + 64, pre[k1]));
            const bool starts = lane < k1 - k0 && pre[min(k0 + lane, nk)] < wend;
            nslot = __popcll(__ballot(starts));
        };
        // Round h of a pass: group cg takes the child of slot 4 h + cg.  Column cc of a child = the parent's column
        // a + cc, a = n - 1 - T' (cc = 0: the pivot column, cc = T' + 1: the rhs).
        auto issue = [&](int k0, int nslot) {   // loads of a pass's columns (no use of the data here)
#pragma unroll
            for (int h = 0; h < kRounds; ++h) {
                if (4 * h < nslot) {   // (wave-uniform; a group without a child repeats the round's first one)
                    const int sl = 4 * h + cg;
                    const unsigned srcw = recs[k0 + (sl < nslot ? sl : 4 * h)].src;
                    const int tp = (int)(srcw >> 8);
                    const double* p = parents + (size_t)(recbase + (int)(srcw & 0xFFu)) * recd + (size_t)(n - 1 - tp - P) * PG + row;
                    // (a column past the rhs is replaced by the pivot column and never used: the load stays unconditional)
#pragma unroll
                    for (int cc = 0; cc < kCols; ++cc) stage[h * kCols + cc] = p[(cc <= tp + 1) ? cc * PG : 0];
                }
            }
        };
        auto commit = [&](int k0, int nslot) {  // the child pivots: registers -> LDS slots, rows permuted: unused rows first
#pragma unroll
            for (int h = 0; h < kRounds; ++h) {
                if (4 * h < nslot) {
                    const int sl = 4 * h + cg;
                    const bool active = sl < nslot;   // whole groups are active or not
                    const ParentTailRec tr = recs[k0 + (active ? sl : 4 * h)];
                    const int tp = (int)(tr.src >> 8), src = (int)(tr.src & 0xFFu);
                    const bool prow_used = (row >= m) || ((tr.used >> row) & 1u);
                    const double w = stage[h * kCols];   // the pivot column a
                    double big;
                    const int p = pick_pivot_row(w, prow_used, gbase, big);
                    const double pmin = s_par[wave][src][0], pmax = s_par[wave][src][1];
                    const double minp = fmin(pmin, big), maxp = fmax(pmax, big);
                    const bool pruned = !(big > 0.0) || minp <= epsm * maxp;
                    const int addr = (gbase + p) << 2;
                    const double piv = bcast16(w, addr);
                    const double inv = 1.0 / piv;
                    const bool isp = (row == p);
                    const double lx = isp ? inv : -(w * inv);
                    const unsigned usedc = (tr.used | (1u << p)) & all, freem = ~usedc & all;
                    const int pos = (row >= m) ? row
                                    : ((freem >> row) & 1u) ? __builtin_popcount(freem & below)
                                                            : __builtin_popcount(freem) + __builtin_popcount(usedc & below);
                    double* q = slots + sl * kSlot + pos;
#pragma unroll
                    for (int cc = 1; cc < kCols; ++cc) {
                        const double v = stage[h * kCols + cc];
                        const double pe = bcast16(v, addr);   // the pivot row's entry (every lane of the wave takes part)
                        if (active && cc <= tp + 1) q[(cc - 1) * TS] = fma(lx, pe, isp ? -0.0 : v);
                    }
                    if (active && row == 0) {
                        s_mm[wave][sl][0] = minp;
                        s_mm[wave][sl][1] = pruned ? -1.0 : maxp;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };
        int k0 = 0, w0 = 0, nslot, wend;
        plan(k0, w0, nslot, wend);
        issue(k0, nslot);
        for (;;) {
            commit(k0, nslot);
            // (as in k_enum_thin: every staged load has landed; the explicit wait keeps the next pass's loads from
            // waiting for each other through the reuse of the staging registers)
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_waitcnt(kWaitVm0);
            const int kn = k0 + nslot - (pre[k0 + nslot] == wend ? 0 : 1);
            const bool more = wend < total;
            int nslotN = 0, wendN = 0;
            if (more) {
                plan(kn, wend, nslotN, wendN);
                issue(kn, nslotN);
            }
            // ---- one subset per lane
            const int w = w0 + lane;
            int s = 0;
            for (int q = 1; q < nslot; ++q) s += (pre[k0 + q] <= w) ? 1 : 0;
            const ParentTailRec tr = recs[k0 + s];
            const int tp = (int)(tr.src >> 8);
            const double minp0 = s_mm[wave][s][0], maxp0 = s_mm[wave][s][1];
            const int j = w - pre[k0 + s];
            int verdict = -1;
            unsigned long long rank = 0ULL;
            if (w < wend) {
                rank = tr.rank0 + (unsigned long long)j;
                if (rank >= begin && rank < end) {
                    if (maxp0 < 0.0) {
                        verdict = 2;   // below a child the level kernel prunes
                    } else {
                        const unsigned pk = s_comb[tail_comb_off(tp) + j];
                        int c[KD];
#pragma unroll
                        for (int t = 0; t < KD; ++t) c[t] = (int)((pk >> (4 * t)) & 15u);
                        const int U[KD] = {0, 1, 2, 3, 4, 5, 6};   // unused by leaf_verdict<PERM>
                        verdict = leaf_verdict<KD, TS, true, false, !EXACT, false>(slots + s * kSlot, c, tp, U, 0u, minp0, maxp0,
                                                                                   m, nullptr, &viol);
                    }
                }
            }
            if (verdict == 0) {
                const unsigned long long at = atomicAdd(pd.list_count, 1ULL);
                if (at < pd.list_cap) {
                    pd.list[at] = rank;
                    pd.list_rec[at] = -1;
                }
            }
            cnt[0] += verdict == 0;
            cnt[1] += verdict == 1;
            cnt[2] += verdict == 2;
            if (!more) break;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();   // (the slots are rewritten by the next pass)
            k0 = kn;
            w0 = wend;
            nslot = nslotN;
            wend = wendN;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();   // (the list is rewritten by the next batch)
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        unsigned int c = cnt[v];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if ((tid & 63) == 0 && c) atomicAdd(&s_cnt[v], (unsigned long long)c);
    }
    if (!EXACT && viol) atomicOr(&d.result->range_flag, 1ULL);
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(&d.result->counts[tid], s_cnt[tid]);
}

// Table 0 by quarters of a wave (LP_ENUM_LEAF_QUADS): k_enum_leaves<1>'s work with k_enum_parent_tails' front end.
// A table-0 entry is ONE child (record, child column a, first subset of the tail, rank offset of the child); a wave
// takes rounds of up to four consecutive entries, from the same or from different records.  Group cg (lanes 16 cg ..
// 16 cg + 15, lane = row) loads its child's pivot column, its last min(R, kGrandMin) columns and the rhs — at most
// twelve 128-byte lines, one round ahead, nothing of the record is staged in LDS — and pivots from the registers with
// k_enum_leaves<1>'s arithmetic, operand for operand: pick_pivot_row over the rows the record left unused, 1.0 / piv,
// lx = isp ? inv : -(w * inv), fma(lx, pe, isp ? -0.0 : v) with the pivot row's entry pe broadcast inside the group.
// The child's columns go to the group's LDS slot (column j of the child at slot column j - (R - min(R, kGrandMin)))
// with the rows permuted, unused rows first.  A child the level kernel would have pruned counts its subsets inside
// [begin, end) as singular, once, and contributes no lanes.
// The slots are two halves of four: the rounds of a wave form one stream of subsets, and a pass of 64 consecutive
// subsets may end in the next round's half, which is committed when fewer than 64 subsets of the current round are
// left — so every pass but a wave's last is full (k_enum_leaves<1>: a single 84-subset child is two passes at 66 %).
// Every lane finds its slot by the prefix sums of the round's tails and runs leaf_verdict as k_enum_leaves<1> does.
// Dealing: k_enum_leaves<1>'s runs (static first deal, fixed runs in LDS taken by compare-and-swap, the siblings'
// runs at the end, s_dry), a round at a time; a run is kQuadRun entries, two whole rounds.
constexpr int kQuadCols = kGrandMin + 1;                 // columns of a slot: the child's last kGrandMin and the rhs
constexpr int kQuadSlot = (kQuadCols * TS) | 1;          // doubles per slot (odd: see tail_slot)
#ifndef LP_QUAD_RUN   // measurement builds: entries per run (a multiple of four: whole rounds)
#define LP_QUAD_RUN 8
#endif
constexpr int kQuadRun = LP_QUAD_RUN;
static_assert(kQuadRun >= 4 && kQuadRun % 4 == 0, "a run is a whole number of rounds");
// What a lane needs of its slot, in one read: subset w of the round (pre <= w < pre + the entry's count) is subset
// leaf = leaf0 + (w - pre) of the child, so rank, subset-table index and tableau address are w plus a constant.
struct alignas(8) QuadSlot {
    unsigned long long rank0;   // rank of subset w = rank0 + w
    double minp, maxp;          // smallest / largest |pivot| down to the child
    int comb0;                  // its entry of pd.comb6 = comb0 + w
    int tab0;                   // the child's column 0 (slots + tab0; the slot holds columns R - min(R, kGrandMin) .. R)
    int R;                      // selectable columns of the child
    int rec;                    // depth m-7 record (list_rec)
};

template <bool EXACT>
__global__ __launch_bounds__(LEAF_THREADS) __attribute__((amdgpu_waves_per_eu(3)))
void k_enum_leaves_quads(EnumDev d, PrefixDev pd, const double* __restrict__ roots, unsigned long long begin,
                         unsigned long long end) {
    constexpr int KD = 6;
    __shared__ __attribute__((aligned(16))) double s_slot[LEAF_WAVES][8 * kQuadSlot];
    __shared__ QuadSlot s_q[LEAF_WAVES][8];
    __shared__ unsigned int s_b6[NMX + KD + 2];   // C(r, 6)
    __shared__ unsigned long long s_cnt[3];
    __shared__ unsigned int s_off[32];            // offsets of the per-R subset tables inside pd.comb6
    __shared__ unsigned int s_rows[36];           // leaf_row_table<6>
    __shared__ unsigned long long s_run[LEAF_WAVES];
    __shared__ int s_dry;
    const int m = d.m, n = d.n, D = m - KD - 1;   // depth of the records
    const int4* const items = pd.items;
    const int nitems = min(pd.item_count[0], pd.item_cap);
    int* const cursor = pd.root_cursor;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & (PG - 1), cg = lane >> 4, gbase = lane & ~(PG - 1);
    if (tid < NMX + KD + 2) s_b6[tid] = (unsigned int)d.binom[tid * kBinomK + KD];
    if (tid < 3) s_cnt[tid] = 0ULL;
    if (tid < 32) s_off[tid] = pd.comb6[tid];
    leaf_row_table<KD>(s_rows, tid);
    const int nwaves = (int)gridDim.x * LEAF_WAVES;
    // the first deal is static, whole rounds where the table is long enough
    const int share = nitems / (nwaves * 4);
    const int k0 = share >= kQuadRun ? kQuadRun : share >= 4 ? 4 : max(1, share);
    const int dyn_base = nwaves * k0;
    auto pack_run = [](int next, int end_) { return ((unsigned long long)(unsigned)next << 32) | (unsigned)end_; };
    {
        const int first = ((int)blockIdx.x * LEAF_WAVES + wave) * k0;
        if (lane == 0) s_run[wave] = pack_run(min(first, nitems), min(first + k0, nitems));
        if (tid == 0) s_dry = 0;
    }
    __syncthreads();
    unsigned int cnt[3] = {0u, 0u, 0u};
    unsigned int viol = 0;
    // up to four entries of wave w's run: first entry (-1: the run is empty), count in nE
    auto take = [&](int w, int& nE) {
        int first = -1, k = 0;
        if (lane == 0) {
            unsigned long long cur = __hip_atomic_load(&s_run[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            while ((unsigned)(cur >> 32) < (unsigned)cur) {
                const unsigned left = (unsigned)cur - (unsigned)(cur >> 32);
                const unsigned kk = left < 4u ? left : 4u;
                if (__hip_atomic_compare_exchange_strong(&s_run[w], &cur, cur + ((unsigned long long)kk << 32), __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                    first = (int)(cur >> 32);
                    k = (int)kk;
                    break;
                }
            }
        }
        nE = __builtin_amdgcn_readfirstlane(k);
        return __builtin_amdgcn_readfirstlane(first);
    };
    bool dry = dyn_base >= nitems, none = false;
    auto draw = [&](int& nE) {   // the next round: first entry (nitems: nothing left) and its number of entries
        nE = 0;
        if (none) return nitems;
        int first = take(wave, nE);
        if (first >= 0) return first;
        if (!dry && __hip_atomic_load(&s_dry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) dry = true;
        if (!dry) {
            int v = 0, over = 0;
            if (lane == 0) {
                v = atomicAdd(cursor, kQuadRun);
                // (a list far beyond its capacity: the caller switches to the dense form, the waves stop drawing)
                over = __hip_atomic_load(pd.list_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > pd.list_abort;
            }
            v = __builtin_amdgcn_readfirstlane(v) + dyn_base;
            if (__builtin_amdgcn_readfirstlane(over)) v = nitems;
            if (v < nitems) {
                nE = min(4, nitems - v);
                if (lane == 0)
                    __hip_atomic_store(&s_run[wave], pack_run(v + nE, min(v + kQuadRun, nitems)), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                return v;
            }
            dry = true;
            if (lane == 0) __hip_atomic_store(&s_dry, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        for (int q = 1; q < LEAF_WAVES; ++q) {
            first = take((wave + q) & (LEAF_WAVES - 1), nE);
            if (first >= 0) return first;
        }
        none = true;
        nE = 0;
        return nitems;
    };
    const size_t recd = rec_doubles(n, D);
    const int rec_cols = n - D + 1;
    const unsigned all = (1u << m) - 1u, below = (1u << row) - 1u;
    const double epsm = DBL_EPSILON * (double)m;
    double* const slots = s_slot[wave];
    QuadSlot* const sq = s_q[wave];
    // Three rounds are under way: D, drawn, record and child column of its entries in flight (itD); N, its columns in
    // flight (stage) or already committed to the half the current round does not use; C, the current round, in half
    // `half`.  What else a pivot needs — the rest of the entry word and the record's metadata, lines this wave has
    // loaded a round earlier — is read at the commit: held across the passes it cost the lanes' loop its registers.
    int2 itD = make_int2(0, 0), itN = make_int2(0, 0);
    int nD = 0, nN = 0, firstD = 0, firstN = 0;
    double stage[kQuadCols + 1] = {};
    auto fetch_words = [&]() {   // round D's entries (a group without an entry repeats the round's last one)
        int nE;
        firstD = draw(nE);
        nD = nE;
        if (nE > 0) itD = *reinterpret_cast<const int2*>(items + firstD + min(cg, nE - 1));
    };
    auto issue = [&]() {   // round D becomes round N: loads of its columns (no use of the data here)
        itN = itD;
        nN = nD;
        firstN = firstD;
        if (nN == 0) return;
        const double* Q = roots + (size_t)itN.x * recd;
        const int a = itN.y & 0xFF, R = n - 1 - a, jlo = max(R - kGrandMin, 0);
        const double* p = Q + (size_t)(a - D) * PG + row;   // the pivot column; child column j = record column a + 1 + j
        stage[0] = p[0];
        // (a column past the rhs is replaced by the pivot column and never used: the load stays unconditional)
#pragma unroll
        for (int k = 0; k < kQuadCols; ++k) stage[1 + k] = p[(k <= R - jlo) ? (1 + jlo + k) * PG : 0];
    };
    // round N's child pivots: registers -> the four slots of half h, rows permuted: unused rows first.  pre[k]: the
    // round's subsets inside [begin, end) below children that are not pruned, in front of entry k + 1; returns their total.
    auto commit = [&](int h, int (&pre)[3]) {
        const bool active = cg < nN;   // whole groups are active or not
        const int2 lo_roff = *reinterpret_cast<const int2*>(&items[firstN + min(cg, nN - 1)].z);
        const NodeMeta* pm = reinterpret_cast<const NodeMeta*>(roots + (size_t)itN.x * recd + (size_t)PG * rec_cols);
        const unsigned long long rbN = pm->rank_base;
        const double minN = pm->minp, maxN = pm->maxp;
        const unsigned usedN = pm->used_mask;   // (the item builder makes no entry for a hole)
        const int a = itN.y & 0xFF, R = n - 1 - a, jlo = max(R - kGrandMin, 0);
        const bool prow_used = (row >= m) || ((usedN >> row) & 1u);
        const double w = stage[0];
        double big;
        const int p = pick_pivot_row(w, prow_used, gbase, big);
        const double minp = fmin(minN, big), maxp = fmax(maxN, big);
        const bool pruned = !(big > 0.0) || minp <= epsm * maxp;
        const int addr = (gbase + p) << 2;
        const double piv = bcast16(w, addr);
        const double inv = 1.0 / piv;
        const bool isp = (row == p);
        const double lx = isp ? inv : -(w * inv);
        const unsigned usedc = (usedN | (1u << p)) & all, freem = ~usedc & all;
        const int pos = (row >= m) ? row
                        : ((freem >> row) & 1u) ? __builtin_popcount(freem & below)
                                                : __builtin_popcount(freem) + __builtin_popcount(usedc & below);
        const int sl = 4 * h + cg;
        double* q = slots + sl * kQuadSlot + pos;
#pragma unroll
        for (int k = 0; k < kQuadCols; ++k) {
            const double v = stage[1 + k];
            const double pe = bcast16(v, addr);   // the pivot row's entry (every lane of the wave takes part)
            if (active && k <= R - jlo) q[k * TS] = fma(lx, pe, isp ? -0.0 : v);
        }
        // the entry's subsets [lo, L) of the child, clipped to the range
        const unsigned long long rb = rbN + (unsigned long long)(unsigned)lo_roff.y;
        const unsigned int L = s_b6[R >= 0 ? R : 0], lo = (unsigned int)lo_roff.x;
        const unsigned long long r0 = rb + lo;
        unsigned int ov = (active && R >= KD && lo < L) ? (unsigned int)overlap(r0, L - lo, begin, end) : 0u;
        const unsigned int skip = begin > r0 ? (unsigned int)(begin - r0) : 0u;
        if (pruned) {
            if (row == 0) cnt[2] += ov;   // every subset below this child is singular
            ov = 0u;
        }
        const int c0 = __builtin_amdgcn_readlane((int)ov, 0), c1 = __builtin_amdgcn_readlane((int)ov, 16),
                  c2 = __builtin_amdgcn_readlane((int)ov, 32), c3 = __builtin_amdgcn_readlane((int)ov, 48);
        const int pre_e = cg == 0 ? 0 : cg == 1 ? c0 : cg == 2 ? c0 + c1 : c0 + c1 + c2;
        if (row == 0) {
            const int d0 = (int)(lo + skip) - pre_e;   // leaf - w
            QuadSlot s;
            s.rank0 = rb + (unsigned long long)(long long)d0;
            s.minp = minp;
            s.maxp = maxp;
            s.comb0 = (int)s_off[R] + d0;
            s.tab0 = sl * kQuadSlot - jlo * TS;
            s.R = R;
            s.rec = itN.x;
            sq[sl] = s;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        pre[0] = c0;
        pre[1] = c0 + c1;
        pre[2] = c0 + c1 + c2;
        return c0 + c1 + c2 + c3;
    };
    fetch_words();
    // (the loop starts as if an empty round N had been committed behind an empty current one: its first two turns
    // issue and commit the wave's first round through the same code as every other)
    int half = 0, totC = 0, totN = 0, w0 = 0;
    int preC[3] = {0, 0, 0}, preN[3] = {0, 0, 0};
    bool committedN = true;
    const int U[KD] = {0, 1, 2, 3, 4, 5};        // unused by leaf_verdict<PERM>
    for (;;) {
        if (totC - w0 < 64 && nN > 0 && !committedN) {
            // fewer than 64 subsets of the current round are left: the next pass runs on into round N
            // (the half it is written to held the round before the current one: no lane reads it any more)
            totN = commit(half ^ 1, preN);
            committedN = true;
        }
        if (w0 >= totC) {   // the current round is finished: round N takes its place
            if (!committedN) break;   // (there is none)
            w0 -= totC;
            half ^= 1;
            totC = totN;
#pragma unroll
            for (int q = 0; q < 3; ++q) preC[q] = preN[q];
            totN = 0;
            committedN = false;
            issue();
            fetch_words();
            continue;
        }
        const int avail = totC - w0 + (committedN ? totN : 0);
        const int len = avail < 64 ? avail : 64;
        // ---- one subset per lane
        int verdict = -1;
        unsigned long long rank = 0ULL;
        int rec = 0;
        if (lane < len) {
            const int w = w0 + lane;
            const bool inN = w >= totC;
            const int wl = inN ? w - totC : w;
            const int s = (wl >= (inN ? preN[0] : preC[0]) ? 1 : 0) + (wl >= (inN ? preN[1] : preC[1]) ? 1 : 0) +
                          (wl >= (inN ? preN[2] : preC[2]) ? 1 : 0);
            const QuadSlot e = sq[4 * (inN ? half ^ 1 : half) + s];
            rank = e.rank0 + (unsigned long long)(unsigned)wl;
            rec = e.rec;
            const unsigned pk = comb_word(pd.comb6, (unsigned)(e.comb0 + wl));   // (the index of a lane's own subset: >= 0)
            int c[KD];
#pragma unroll
            for (int t = 0; t < KD; ++t) c[t] = (int)((pk >> (5 * t)) & 31u);
            verdict = leaf_verdict<KD, TS, true, false, !EXACT, true>(slots + e.tab0, c, e.R, U, 0u, e.minp, e.maxp, m, nullptr,
                                                                      &viol, s_rows);
        }
        if (verdict == 0) {
            const unsigned long long at = atomicAdd(pd.list_count, 1ULL);
            if (at < pd.list_cap) {
                pd.list[at] = rank;
                pd.list_rec[at] = rec;
            }
        }
        cnt[0] += verdict == 0;
        cnt[1] += verdict == 1;
        cnt[2] += verdict == 2;
        w0 += len;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();   // (the other half is rewritten once this round is finished)
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        unsigned int c = cnt[v];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if (lane == 0 && c) atomicAdd(&s_cnt[v], (unsigned long long)c);
    }
    if (!EXACT && viol) atomicOr(&d.result->range_flag, 1ULL);
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(&d.result->counts[tid], s_cnt[tid]);
}

// ---------------------------------------------------------------------------------------------
// The general leaf kernel: ANY record height (PGT = 16 or 32 rows) and any number of selectable
// columns.  The three kernels above are tuned for m <= 16, n - m <= 16 (subset tables, LDS slices
// sized for 24 columns, 16-lane cooperative pivots); shapes outside that box used to fall to the
// from-scratch solver of enum_direct.hip at ~2 ns per subset.  Here a wave takes an item = (depth
// m-7 record, run of consecutive subsets of its C(R,7)); every lane unranks the first subset of its
// own contiguous share once (binomials from LDS), then walks lexicographic successors, reading the
// record where it lies (L1/L2: a record is at most 40 x 32 doubles) — leaf_verdict<7, PGT, false>,
// the arithmetic of the thin kernel.
constexpr int kGenChunk = 2048;   // subsets per item (32 per lane)
// max n - m of the general path: 32-row records (m > 16) with n <= 64 leave n - m <= 47 — the host
// admits 32 there; 16-row records (7 <= m <= 16) go up to n - m = 57
constexpr int nmxw(int pgt) { return pgt == 16 ? 57 : 32; }

template <int PGT>
__global__ __launch_bounds__(256) void k_enum_generic_items(EnumDev d, PrefixDev pd,
                                                            const double* __restrict__ roots, int root_level,
                                                            int root_cap, unsigned long long begin,
                                                            unsigned long long end) {
    constexpr int KD = 7;
    const int n = d.n, m = d.m, D = m - KD;
    const int nrec = min(pd.level_counts[root_level], root_cap);
    const int rec = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long lo0 = 0, hi0 = 0;
    if (rec < nrec) {
        const NodeMetaT<PGT>* pm = reinterpret_cast<const NodeMetaT<PGT>*>(roots + (size_t)rec * rec_doubles_g<PGT>(n, D, d.rs) +
                                                               (size_t)rec_rs<PGT>(d.rs) * (n - D + 1));
        const int last = pm->last_col;
        const int R = n - 1 - last;
        if (last != kHole && R >= KD) {
            const unsigned long long rb = pm->rank_base, L = binom(d, R, KD);
            const unsigned long long lo = rb > begin ? rb : begin, hi = rb + L < end ? rb + L : end;
            if (hi > lo) {
                lo0 = lo - rb;
                hi0 = hi - rb;
            }
        }
    }
    const int nitem = (int)((hi0 - lo0 + kGenChunk - 1) / kGenChunk);
    int at = nitem ? atomicAdd(&pd.item_count[0], nitem) : 0;
    for (int k = 0; k < nitem; ++k, ++at) {
        const unsigned long long lo = lo0 + (unsigned long long)k * kGenChunk;
        const unsigned long long cnt = hi0 - lo < (unsigned long long)kGenChunk ? hi0 - lo : (unsigned long long)kGenChunk;
        if (at < pd.item_cap) pd.items[at] = make_int4(rec, (int)lo, (int)cnt, 0);
    }
}

// DENSE (a degenerate LP: a large part of the range is feasible): no list — every subset is finished
// without the early exit, its objective summed as the direct solver sums it, and its score (-inf if
// not feasible) written to dense_scores[rank - begin]; the tie rule then runs over that array.
template <int PGT, bool DENSE, bool EXACT>
__global__ __launch_bounds__(LEAF_THREADS) __attribute__((amdgpu_waves_per_eu(3))) void k_enum_generic_leaves(EnumDev d, PrefixDev pd,
                                                                       const double* __restrict__ roots,
                                                                       unsigned long long range_subsets,
                                                                       unsigned long long begin) {
    constexpr int KD = 7;
    constexpr int TSG = PGT + 1;                 // LDS column stride (odd: rows of different columns, different banks)
    constexpr int NMXW = nmxw(PGT);
    constexpr int GCOLS = NMXW + KD + 1;         // <= n - m + 7 selectable columns + rhs
    __shared__ unsigned int s_bin[(NMXW + KD + 2) * (KD + 1)];   // C(r, k), r <= NMXW + KD + 1, k <= KD
    __shared__ unsigned long long s_cnt[3];
    // the item's record, one private slice per wave, rows PERMUTED: the 7 rows the prefix has not used
    // first (ascending), then the used ones — leaf_verdict<PERM> then reads every row at a
    // compile-time offset (no per-lane gathers from HBM/L1: those, ~100 per subset at a quarter of
    // the LDS rate, bounded the first version of this kernel at 14 G subsets/s on C(32,16))
    __shared__ double s_rec[LEAF_WAVES][GCOLS * TSG];
    __shared__ double s_cost[DENSE ? kEnumMaxN : 1];
    __shared__ unsigned long long s_best;
    __shared__ unsigned long long s_run[LEAF_WAVES];   // every wave's run of work items {next, end}
    __shared__ int s_dry;                              // a wave of this workgroup has seen the end of the item table
    double best = -INFINITY;
    const int m = d.m, n = d.n, D = m - KD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < (NMXW + KD + 2) * (KD + 1); k += LEAF_THREADS) {
        const int r = k / (KD + 1), kk = k - r * (KD + 1);
        s_bin[k] = (unsigned int)d.binom[r * kBinomK + kk];
    }
    if (tid < 3) s_cnt[tid] = 0ULL;
    if (DENSE && tid < d.n) s_cost[tid] = d.c[tid];
    if (tid == 0) s_best = lp_f64_key(-INFINITY);
    __syncthreads();
    const int nitems = min(pd.item_count[0], pd.item_cap);
    unsigned int viol = 0;
    unsigned int cnt[3] = {0u, 0u, 0u};
    double* tab = s_rec[wave];
    int staged = -1;   // record in this wave's slice
    const int U[KD] = {0, 1, 2, 3, 4, 5, 6};   // unused by leaf_verdict<PERM>
    // Items are dealt in runs (a returning atomic on one word costs ~11 ns chip-wide: at one draw per
    // item, the 1.4 M mostly tiny items of C(30,18) took 15.6 ms whatever the lanes did): a static first
    // deal, then runs of a fixed length — ~1024 subsets on average at most (16 items of tiny records, one full
    // item) — held in LDS and emptied by compare-and-swap, so that a wave that finds the table dealt out takes
    // what the other waves of its workgroup still hold (as k_enum_leaves: runs that shrank towards the end of
    // the table made the last thousands of draws queue on the one word)
    const int kMaxRun = (int)max(1ULL, min(16ULL, 1024ULL * (unsigned long long)max(nitems, 1) / max(range_subsets, 1ULL)));
    const int nwaves = (int)gridDim.x * LEAF_WAVES;
    const int k0 = max(1, min(kMaxRun, nitems / (nwaves * 4)));
    const int dyn_base = nwaves * k0;
    auto pack_run = [](int next, int end) { return ((unsigned long long)(unsigned)next << 32) | (unsigned)end; };
    {
        const int first = ((int)blockIdx.x * LEAF_WAVES + wave) * k0;
        if (lane == 0) s_run[wave] = pack_run(min(first, nitems), min(first + k0, nitems));
        if (tid == 0) s_dry = 0;
    }
    __syncthreads();
    auto take = [&](int w) {   // the next item of wave w's run, -1 if it is empty
        int item = -1;
        if (lane == 0) {
            unsigned long long cur = __hip_atomic_load(&s_run[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            while ((unsigned)(cur >> 32) < (unsigned)cur) {
                if (__hip_atomic_compare_exchange_strong(&s_run[w], &cur, cur + (1ULL << 32), __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                    item = (int)(cur >> 32);
                    break;
                }
            }
        }
        return __builtin_amdgcn_readfirstlane(item);
    };
    bool dry = dyn_base >= nitems;   // the table is dealt out
    auto draw = [&]() {
        int item = take(wave);
        if (item >= 0) return item;
        if (!dry && __hip_atomic_load(&s_dry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) dry = true;
        if (!dry) {
            const int k = kMaxRun;
            int v = 0, over = 0;
            if (lane == 0) {
                v = atomicAdd(&pd.root_cursor[0], k);
                if (!DENSE)   // (a list far beyond its capacity: the caller switches to the dense form)
                    over = __hip_atomic_load(pd.list_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > pd.list_abort;
            }
            v = __builtin_amdgcn_readfirstlane(v) + dyn_base;
            if (__builtin_amdgcn_readfirstlane(over)) v = nitems;
            if (v < nitems) {
                if (k > 1 && lane == 0)
                    __hip_atomic_store(&s_run[wave], pack_run(v + 1, min(v + k, nitems)), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                return v;
            }
            dry = true;
            if (lane == 0) __hip_atomic_store(&s_dry, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        for (int q = 1; q < LEAF_WAVES; ++q) {
            item = take((wave + q) & (LEAF_WAVES - 1));
            if (item >= 0) return item;
        }
        return nitems;
    };
    for (;;) {
        const int item = draw();
        if (item >= nitems) break;
        const int4 it = pd.items[item];
        const int rec = __builtin_amdgcn_readfirstlane(it.x);
        const double* Q = roots + (size_t)rec * rec_doubles_g<PGT>(n, D, d.rs);
        const int RS = rec_rs<PGT>(d.rs);   // row stride of the record's columns in HBM
        const NodeMetaT<PGT>* pm = reinterpret_cast<const NodeMetaT<PGT>*>(Q + (size_t)RS * (n - D + 1));
        const int last = __builtin_amdgcn_readfirstlane(pm->last_col);
        const int R = n - 1 - last;
        const unsigned umask = __builtin_amdgcn_readfirstlane(pm->used_mask);
        const unsigned long long rb = pm->rank_base;
        const double minp0 = pm->minp, maxp0 = pm->maxp;
        if (rec != staged) {
            // columns last+1 .. n-1 and the rhs, RS rows each: 64 / PGT columns per round, a lane's row is
            // the same in every round
            const int row = lane & (PGT - 1), cl = lane / PGT;
            const unsigned all = m >= 32 ? ~0u : ((1u << m) - 1u), below = (1u << row) - 1u, freem = ~umask & all;
            const int pos = (row >= m) ? row
                            : ((freem >> row) & 1u) ? __builtin_popcount(freem & below)
                                                    : __builtin_popcount(freem) + __builtin_popcount(umask & all & below);
            const double* src = Q + (size_t)(last + 1 - D) * RS;
            __builtin_amdgcn_wave_barrier();   // (the previous item's reads of the slice are done)
            if (row < RS)
                for (int col = cl; col <= R; col += 64 / PGT) tab[col * TSG + pos] = src[(size_t)col * RS + row];
            __builtin_amdgcn_wave_barrier();
            staged = rec;
        }
        // this lane's share: K consecutive subsets from `mine`
        const unsigned int total = (unsigned int)it.z;
        const unsigned int K = (total + 63u) / 64u;
        const unsigned int mine = (unsigned int)it.y + (unsigned int)lane * K;
        const unsigned int have = (unsigned int)lane * K < total ? min(K, total - (unsigned int)lane * K) : 0u;
        int c[KD];
        {
            unsigned int left = have ? mine : 0u;
            int j = 0;
#pragma unroll
            for (int t = 0; t < KD; ++t) {
                for (;; ++j) {
                    const unsigned int cn = s_bin[(R - 1 - j) * (KD + 1) + (KD - 1 - t)];
                    if (left < cn) break;
                    left -= cn;
                }
                c[t] = j++;
            }
        }
        for (unsigned int k = 0; k < K; ++k) {
            if (k < have) {
                int verdict;
                if constexpr (DENSE) {
                    LeafObj obj;
                    obj.cost = s_cost;
                    obj.prow = pm->prow;
                    obj.pcol = pm->pcol;
                    obj.D = D;
                    obj.col0 = last + 1;
                    obj.used = umask;
                    obj.stride = TSG;
                    obj.z = 0.0;
                    verdict = leaf_verdict<KD, TSG, true, true>(tab, c, R, U, 0u, minp0, maxp0, m, &obj);
                    const double score = verdict == 0 ? (d.maximize ? obj.z : -obj.z) : -INFINITY;
                    pd.dense_scores[rb + mine + k - begin] = score;
                    best = fmax(best, score);
                } else {
                    verdict = leaf_verdict<KD, TSG, true, false, !EXACT>(tab, c, R, U, 0u, minp0, maxp0, m, nullptr, &viol);
                    if (verdict == 0) {
                        const unsigned long long at = atomicAdd(pd.list_count, 1ULL);
                        if (at < pd.list_cap) {
                            pd.list[at] = rb + mine + k;
                            pd.list_rec[at] = rec;
                        }
                    }
                }
                cnt[0] += verdict == 0;
                cnt[1] += verdict == 1;
                cnt[2] += verdict == 2;
                // lexicographic successor inside {0 .. R-1}
                int tpos = -1;
#pragma unroll
                for (int t = 0; t < KD; ++t)
                    if (c[t] < R - KD + t) tpos = t;
#pragma unroll
                for (int t = 0; t < KD; ++t) {
                    if (t == tpos)
                        c[t] += 1;
                    else if (t > tpos && t > 0)
                        c[t] = c[t - 1] + 1;
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        unsigned int x = cnt[v];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
        if (lane == 0 && x) atomicAdd(&s_cnt[v], (unsigned long long)x);
    }
    if (DENSE && best > -INFINITY) atomicMax(&s_best, lp_f64_key(best));
    if (!DENSE && !EXACT && viol) atomicOr(&d.result->range_flag, 1ULL);
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(&d.result->counts[tid], s_cnt[tid]);
    if (DENSE && tid == 0 && s_best != lp_f64_key(-INFINITY)) atomicMax(&d.result->best_key, s_best);
}

// Objectives of the listed (feasible) subsets from the depth m-7 records they were found under: one
// lane per list entry.  The lane unranks its 7 remaining columns inside the record, repeats the
// leaf's arithmetic (leaf_verdict<7, PG, false, OBJ>: the operations, operand for operand, of the
// direct solver, so the score is the one k_enum_eval_list would produce) and keeps every row's
// value for the objective — ~1/15 of the price of a from-scratch m x m solve per entry, which is
// what a degenerate LP (every non-singular basis feasible: hundreds of millions of entries) pays.
template <int PGT>
__global__ __launch_bounds__(LEAF_THREADS) void k_enum_eval_records(EnumDev d, PrefixDev pd,
                                                                     const double* __restrict__ roots,
                                                                     double* __restrict__ scores) {
    constexpr int KD = 7;
    constexpr int NMXW = nmxw(PGT);
    __shared__ unsigned int s_bin[(NMXW + KD + 2) * (KD + 1)];   // C(r, k), r <= NMXW + KD + 1, k <= KD
    __shared__ double s_cost[kEnumMaxN];
    __shared__ unsigned long long s_best;
    const int m = d.m, n = d.n, D = m - KD;
    const int tid = threadIdx.x;
    for (int k = tid; k < (NMXW + KD + 2) * (KD + 1); k += LEAF_THREADS) {
        const int r = k / (KD + 1), kk = k - r * (KD + 1);
        s_bin[k] = (unsigned int)d.binom[r * kBinomK + kk];
    }
    if (tid < n) s_cost[tid] = d.c[tid];
    if (tid == 0) s_best = lp_f64_key(-INFINITY);
    __syncthreads();
    const unsigned long long count = *pd.list_count < pd.list_cap ? *pd.list_count : pd.list_cap;
    double best = -INFINITY;
    for (unsigned long long e = (unsigned long long)blockIdx.x * LEAF_THREADS + tid; e < count;
         e += (unsigned long long)gridDim.x * LEAF_THREADS) {
        const unsigned long long rank = pd.list[e];
        const int rec = pd.list_rec[e];
        if (rec < 0) continue;   // found under a narrow node that has no record (k_enum_parent_tails): k_enum_eval_list's
        const double* Q = roots + (size_t)rec * rec_doubles_g<PGT>(n, D, d.rs);
        const int RS = rec_rs<PGT>(d.rs);
        const NodeMetaT<PGT>* pm = reinterpret_cast<const NodeMetaT<PGT>*>(Q + (size_t)RS * (n - D + 1));
        const int last = pm->last_col;
        const int R = n - 1 - last;
        // the 7 remaining columns: lexicographic unranking inside the R selectable ones
        unsigned int left = (unsigned int)(rank - pm->rank_base);
        int c[KD];
        int j = 0;
#pragma unroll
        for (int t = 0; t < KD; ++t) {
            for (;; ++j) {
                const unsigned int cnt = s_bin[(R - 1 - j) * (KD + 1) + (KD - 1 - t)];
                if (left < cnt) break;
                left -= cnt;
            }
            c[t] = j++;
        }
        const unsigned umask = pm->used_mask;
        int U[KD];
        unsigned free_rows = ~umask & (m >= 32 ? ~0u : ((1u << m) - 1u));
#pragma unroll
        for (int r = 0; r < KD; ++r) {
            U[r] = free_rows ? __builtin_ctz(free_rows) : 0;
            free_rows &= free_rows - 1u;
        }
        LeafObj obj;
        obj.cost = s_cost;
        obj.prow = pm->prow;
        obj.pcol = pm->pcol;
        obj.D = D;
        obj.col0 = last + 1;
        obj.used = umask;
        obj.stride = RS;
        obj.z = 0.0;
        const double* tab = Q + (size_t)(last + 1 - D) * RS;   // column q = column last+1+q
        const int verdict = leaf_verdict<KD, (PGT == 32 ? 0 : PGT), false, true>(tab, c, R, U, umask, pm->minp, pm->maxp, m, &obj);
        // (listed subsets are feasible by construction; a verdict mismatch would be a bug and shows
        // up as -inf here)
        const double score = verdict == 0 ? (d.maximize ? obj.z : -obj.z) : -INFINITY;
        scores[e] = score;
        best = fmax(best, score);
    }
    if (best > -INFINITY) atomicMax(&s_best, lp_f64_key(best));
    __syncthreads();
    if (tid == 0 && s_best != lp_f64_key(-INFINITY)) atomicMax(&d.result->best_key, s_best);
}

}  // namespace

// Ranges of fewer depth m-7 records than this keep every record (measured in lp_enum_launch_leaves: an 8-way shard of
// C(32,16), 250 k records, and C(28,14), 116 k, pay for k_enum_parent_tails; the whole C(32,16), 2.04 M, gains) —
// the threshold of kItemLanesNarrow and kChunkWide.  LP_ENUM_PARENT_TAILS=0 / 1 decides for every range.
constexpr uint64_t kParentTailsMinRecords = 300000;
constexpr int kParentTailsPerCu = 2;   // workgroups of k_enum_parent_tails per CU (2 against 1: lp_enum_launch_parent_tails)
bool lp_enum_parent_tails(const lp_enum_problem* p, int shape, bool fused, bool dense, int level, uint64_t records) {
    if (shape != 1 || !fused || dense || level < 1 || p->knobs.parent_tails == 0) return false;
    return p->knobs.parent_tails == 1 || records >= kParentTailsMinRecords;
}
int lp_enum_parent_tails_stop(int n) { return n - 1 - THIN_TAIL; }

// Table 0 by k_enum_leaves_quads (one entry per child, four children pivoted per wave at once) or by
// k_enum_leaves<1> (paired items).  LP_ENUM_LEAF_QUADS=0 / 1 decides for every range; unset, the new kernel runs on
// every range — no threshold: measured on one MI355X against the parent's library, alternating
// (profiles/enum_leaf_quads.json), C(32,16) pass 11.86 -> 11.44 ms wall, slowest shard of a 2- / 4- / 8-way cut 6.43 /
// 3.56 / 1.94 -> 6.16 / 3.40 / 1.87 ms, C(28,14) 1.124 -> 1.122 ms; bench step, 7 runs each: 11.970 -> 11.557 ms
// (-3.45 %; the parent's runs within 0.07 ms).  SQ_INSTS_VALU of table 0's kernel 2.169 -> 2.015 G per pass.
static bool leaf_quads(const lp_enum_problem* p) { return p->knobs.leaf_quads != 0; }

void lp_enum_queue_record_eval(lp_enum_problem* p, const double* roots) {
    lp_context* ctx = p->ctx;
    if (p->dev.m > PG)
        hipLaunchKernelGGL(k_enum_eval_records<32>, (unsigned)ctx->num_cus * 8, LEAF_THREADS, 0, ctx->stream, p->dev,
                           p->prefix, roots, p->prefix.scores);
    else
        hipLaunchKernelGGL(k_enum_eval_records<PG>, (unsigned)ctx->num_cus * 8, LEAF_THREADS, 0, ctx->stream, p->dev,
                           p->prefix, roots, p->prefix.scores);
}

static int leaf_streams(lp_context* ctx) {
    if (!ctx->aux_stream[0]) {
        for (hipStream_t& a : ctx->aux_stream) LP_HIP(ctx, hipStreamCreateWithFlags(&a, hipStreamNonBlocking));
        for (hipEvent_t& ev : ctx->aux_event) LP_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    return LP_OPTIMAL;
}

// The narrow depth m-7 nodes of the pass from the depth m-8 records (`parents`, count in level_counts[level], at most
// `bound`): queued on a stream of its own behind whatever the library's stream holds at this point, so that it runs
// beside what is queued there next, and neither the tail kernel nor the leaf kernels wait for it.  aux_event[3]
// marks its end: lp_enum_launch_leaves makes the library's stream wait for it at the end of the pass.
int lp_enum_launch_parent_tails(lp_enum_problem* p, const double* parents, int bound, int level, uint64_t begin,
                                uint64_t end) {
    lp_context* ctx = p->ctx;
    int rc = leaf_streams(ctx);
    if (rc) return rc;
    hipStream_t sT = ctx->aux_stream[2];
    LP_HIP(ctx, hipEventRecord(ctx->aux_event[3], ctx->stream));   // the parents' level is complete
    LP_HIP(ctx, hipStreamWaitEvent(sT, ctx->aux_event[3], 0));
    // 254-register waves as the tail kernel's: a CU has room for two workgroups, of this kernel or of that one.
    // Measured on one MI355X against the parent's library, alternating (profiles/enum_parent_tails.json), C(32,16):
    //   bound, before the kernel existed (last level without the narrow children, their 16.2 M subsets simply missing):
    //     pass 12.69 -> 10.88 ms wall; last level 1.21 -> 0.47 ms, item builder 1.71 -> 0.77 ms, tail kernel 1.79 -> 0.76 ms
    //     (they run side by side), last level's end to the first leaf block 1.72 -> 0.79 ms
    //   this kernel, pass wall (means of 12, three rounds), parent 12.70 ms:
    //     beside the last level, 2 / 1 workgroups per CU: 11.83 / 12.08 ms;  behind it: 11.96 / 11.90 ms
    //     (kernel trace, beside, 2 per CU: 2.05 ms from the last level's start to the item builder's end — it shares
    //     the CUs' registers with the tail kernel, 1.68 ms instead of 0.76, and the item builder takes 1.56 ms between
    //     them; the leaf kernels start 2.87 ms into the pass instead of 3.75 ms)
    //   its first form (raw columns staged in the slot, all four groups pivot every slot; the tail kernel queued behind
    //   it on one stream, which then started beside the leaf kernels and ended the pass): 13.55 / 13.89 ms beside,
    //   12.91 / 14.35 ms behind
    //   small ranges PAY: slowest 8-way shard 1.94 -> 2.17 ms, C(28,14) 1.12 -> 1.18 ms (their item builder is over in
    //   0.05 ms; this kernel's blocks hold the registers the leaf kernels wait for) — hence kParentTailsMinRecords;
    //   with it the shards of a 2- / 4- / 8-way cut take 6.62 / 3.59 / 1.96 -> 6.44 / 3.55 / 1.94 ms (slowest, two runs)
    //   bench step, 7 runs each: 12.693 -> 11.879 ms (-6.4 %; the parent's runs within 0.18 ms)
    const unsigned grid = (unsigned)std::min<uint64_t>(lp_ceil_div<uint64_t>((uint64_t)std::max(bound, 1), 64 * LEAF_WAVES),
                                                       (uint64_t)ctx->num_cus * kParentTailsPerCu);
    const unsigned long long b = begin, e = end;
    if (p->exact_div)
        hipLaunchKernelGGL((k_enum_parent_tails<true, THIN_TAIL>), grid, LEAF_THREADS, 0, sT, p->dev, p->prefix, parents, level, bound, b, e);
    else
        hipLaunchKernelGGL((k_enum_parent_tails<false, THIN_TAIL>), grid, LEAF_THREADS, 0, sT, p->dev, p->prefix, parents, level, bound, b, e);
    LP_HIP(ctx, hipEventRecord(ctx->aux_event[3], sT));
    return LP_OPTIMAL;
}

// Second phase of the shared-prefix pass over the records of the last breadth-first level
// (`roots`, count in level_counts[level], at most `bound`): depth m-7 records (fused = true: the
// regular kernel pivots once more itself, the thin kernel takes the small tails) or, for m = 6, the
// root record.  `bound6` bounds the number of depth m-6 nodes (sizes the item table).
int lp_enum_launch_leaves(lp_enum_problem* p, const double* roots, int bound, int level, bool fused,
                          int shape, bool dense, bool parent_tails, uint64_t begin, uint64_t end) {
    lp_context* ctx = p->ctx;
    PrefixDev& pd = p->prefix;
    const int n = p->dev.n, m = p->dev.m;
    auto ensure = [&](int4*& items, int& cap, uint64_t want) -> int {
        if ((uint64_t)cap >= want) return LP_OPTIMAL;
        lp_pool_release(ctx, items, sizeof(int4) * (size_t)cap);
        items = nullptr;
        cap = 0;
        size_t got = 0;
        LP_HIP(ctx, lp_pool_alloc(ctx, (void**)&items, sizeof(int4) * want, &got));
        cap = (int)std::min<uint64_t>(got / sizeof(int4), 0x7FFFFFFFULL);
        return LP_OPTIMAL;
    };
    const bool exact = p->exact_div;   // plain divisions (a pass of the fast kernels reported pivots out of range)
    const bool general = shape != 1 || dense;
    if (general) {
        // one item per started run of kGenChunk subsets of a record
        int rc = ensure(pd.items, pd.item_cap, (end - begin) / kGenChunk + (uint64_t)bound + 1024);
        if (rc) return rc;
        const unsigned long long b = begin, e = end;
        const unsigned grid_items = (unsigned)lp_ceil_div(bound, 256), grid = (unsigned)ctx->num_cus * 8;
#define LP_GEN(PGT)                                                                                                      \
    do {                                                                                                                 \
        hipLaunchKernelGGL(k_enum_generic_items<PGT>, grid_items, 256, 0, ctx->stream, p->dev, pd, roots, level, bound, \
                           b, e);                                                                                        \
        if (dense)                                                                                                       \
            hipLaunchKernelGGL((k_enum_generic_leaves<PGT, true, true>), grid, LEAF_THREADS, 0, ctx->stream, p->dev,    \
                               pd, roots, e - b, b);                                                                     \
        else if (exact)                                                                                                  \
            hipLaunchKernelGGL((k_enum_generic_leaves<PGT, false, true>), grid, LEAF_THREADS, 0, ctx->stream, p->dev,   \
                               pd, roots, e - b, b);                                                                     \
        else                                                                                                             \
            hipLaunchKernelGGL((k_enum_generic_leaves<PGT, false, false>), grid, LEAF_THREADS, 0, ctx->stream, p->dev,  \
                               pd, roots, e - b, b);                                                                     \
    } while (0)
        if (shape == 3) LP_GEN(32); else LP_GEN(PG);
#undef LP_GEN
        return LP_OPTIMAL;
    }
    const uint64_t total = lp_host_binom(n, m);
    const uint64_t bound6 = lp_host_binom(n - m + level + 1, level + 1);   // depth m-6 nodes (sizes the item table)
    int rc = ensure(pd.items, pd.item_cap, bound6 + total / kChunk + 1024);
    if (rc) return rc;
    if (fused) {
        // table 1: one item per chunk of a depth m-5 node with >= kGrandMin selectable columns
        // (their last chosen column is < n - kGrandMin: at most C(n - kGrandMin, m - 5) nodes)
        rc = ensure(pd.items2, pd.item_cap2, lp_host_binom(n - kGrandMin, m - 5) + total / kChunk + 1024);
        if (rc) return rc;
    }
    // persistent waves (items are dealt dynamically): as many blocks as are resident
    const int grid6 = ctx->num_cus * 3;
    const unsigned long long b = begin, e = end;
    if (fused) {
        // The three leaf kernels are independent of each other (own item table / work cursor, results
        // through atomics), and the tail kernel does not even need the item tables: they run on three
        // streams, so that the tail kernel runs beside the item builder and every leaf kernel's tail (persistent
        // waves running out of items) is filled by the next kernel's blocks.  The library's stream
        // waits for the other two before anything that follows (list evaluation, result copy).
        rc = leaf_streams(ctx);
        if (rc) return rc;
        hipStream_t s = ctx->stream, sT = ctx->aux_stream[0], s1 = ctx->aux_stream[1];
        const int lanes = bound < 300000 ? kItemLanesNarrow : kItemLanesWide;
        const bool quads = leaf_quads(p);
        // width of a table-1 item (kChunkWide above; LP_ENUM_CHUNK pins it for tests and measurements)
        const int chunk1 = p->knobs.chunk1 ? p->knobs.chunk1 : bound < kChunkWideMinRecords ? kChunk : kChunkWide;
        LP_HIP(ctx, hipEventRecord(ctx->aux_event[0], s));          // the level records are complete
        LP_HIP(ctx, hipStreamWaitEvent(sT, ctx->aux_event[0], 0));
        // The tail kernel needs the level records only, not the item tables: it is launched on its own stream BESIDE
        // the item builder and, on a whole range, is over when the leaf kernels start, which then have every workgroup
        // slot of the chip to themselves.  Its waves hold 254 registers (seven columns per lane), so a CU has room for
        // two of its workgroups: that is the grid.  Nothing depends on it ending first: workgroups of it that are
        // still resident when the leaf kernels' blocks arrive keep their slots until they are done, which costs time
        // only.  Its predecessor (8 lanes per record gathering from HBM) ran behind the item builder, one workgroup per
        // CU beside the leaf kernels, and held a slot of every CU for 9.0 of their 10.9 ms; launched first with 12
        // workgroups per CU it had held the chip while the item builder ran (14.72 -> 14.50 ms, slowest 8-way shard
        // 2.26 -> 2.21 ms), and its grid of 1 / 2 / 3 / 4 per CU gave 13.16 / 13.26 / 13.89 / 13.67 ms, slowest shard
        // 1.92 / 1.95 / 2.01 / 1.99 ms.
        // Measured on one MI355X against that predecessor (profiles/enum_tail.json):
        //   bench step, C(32,16), 7 runs each, alternating: 13.36 -> 13.01 ms (-2.6 %; the predecessor's runs within 0.10 ms)
        //   kernel time of a pass (scripts/ab_enum.py), predecessor 13.03 ms:
        //     beside the item builder, 2 workgroups per CU: THIN_TAIL = 8 / 9 / 10  12.80 / 12.67 / 14.64 ms
        //     THIN_TAIL = 9, 1 / 2 / 4 workgroups per CU: 14.04 / 12.83 / 12.73 ms against 13.18 (8 columns: 14.59 /
        //       12.80 / 12.81) — one per CU is still running when the leaf kernels' blocks arrive and ends the pass;
        //       four are two resident and two waiting, inside the noise of two
        //     alone between the item builder and the leaf kernels, 2 per CU:    12.94 / 12.92 / 13.93 ms
        //       (the tail kernel by itself 0.89 ms at 8 columns, 3.86 ms at 10; the leaf phase behind it 9.84 ms
        //       against 10.91 ms with the old kernel beside it; the item builder beside the tail kernel takes
        //       1.03 ms instead of 0.26 ms, and both end together)
        //     behind the item builder, beside the leaf kernels as its predecessor, 8 columns, 1 / 2 per CU: 14.36 /
        //       13.38 ms, 10 columns 18.2 / 14.5 ms — a workgroup of 254-register waves and 45 KB of LDS finds no room
        //       on a CU that holds three leaf workgroups, and most of the grid ran after table 0's kernel had ended.
        //   small passes (wall, best / mean; predecessor first): C(28,14) 1.131 / 1.147 -> 1.136 / 1.154 ms (bench leg:
        //     kernel 1.129 -> 1.110 and 1.120 -> 1.127 ms in two sessions); slowest of the 8 cost-balanced shards of C(32,16) 1.938 / 1.962 -> 2.004 /
        //     2.032 ms: a shard PAYS 3 % — its item builder is over in 0.05 ms and the tail kernel's blocks are still
        //     there when the leaf kernels start.  Alone behind the item builder: 1.989 / 2.002 ms, C(28,14) 1.161 ms.
        //     Eight columns on ranges of fewer than 300,000 records (a build with both widths): shards 1.935 / 2.029 ms,
        //     but C(28,14) 1.178 / 1.200 ms and its bench leg 1.110 -> 1.148 ms; so one width for every range.
        // (k_enum_parent_tails, which takes the narrow records' work on wide ranges: placements and grids measured in
        // lp_enum_launch_parent_tails; the tail kernel then handles the stored records, all with >= 10 selectable columns)
        const int thin_per_cu = 2;
        const unsigned grid_thin = (unsigned)std::min<uint64_t>(lp_ceil_div<uint64_t>((uint64_t)bound, 64 * LEAF_WAVES), (uint64_t)ctx->num_cus * thin_per_cu);
        if (exact)
            hipLaunchKernelGGL((k_enum_thin<true, THIN_TAIL>), grid_thin, LEAF_THREADS, 0, sT, p->dev, pd, roots, level, bound, b, e);
        else
            hipLaunchKernelGGL((k_enum_thin<false, THIN_TAIL>), grid_thin, LEAF_THREADS, 0, sT, p->dev, pd, roots, level, bound, b, e);
        hipLaunchKernelGGL(k_enum_make_items<true>, lp_ceil_div(bound * lanes, 1024), 1024, 0, s, p->dev, pd,
                           roots, level, bound, THIN_TAIL, lanes, chunk1, quads ? 1 : 0, b, e);
        LP_HIP(ctx, hipEventRecord(ctx->aux_event[1], s));          // both item tables are built
        LP_HIP(ctx, hipStreamWaitEvent(s1, ctx->aux_event[1], 0));
        // both leaf kernels with resident-sized grids (3 workgroups per CU).  (2 for table 1's kernel gives the best
        // single passes — C(28,14) 1.17 against 1.19 ms, C(32,16) 13.2 against 13.3 — but half of the passes then take
        // 14.0-14.1 ms: the average is worse.)
        const int grid2 = grid6, grid1 = grid6;
        if (exact) {
            hipLaunchKernelGGL((k_enum_leaves<3, true>), grid2, LEAF_THREADS, 0, s, p->dev, pd, roots, chunk1, b, e);
            if (quads)
                hipLaunchKernelGGL((k_enum_leaves_quads<true>), grid1, LEAF_THREADS, 0, s1, p->dev, pd, roots, b, e);
            else
                hipLaunchKernelGGL((k_enum_leaves<1, true>), grid1, LEAF_THREADS, 0, s1, p->dev, pd, roots, kChunk, b, e);
        } else {
            hipLaunchKernelGGL((k_enum_leaves<3, false>), grid2, LEAF_THREADS, 0, s, p->dev, pd, roots, chunk1, b, e);
            if (quads)
                hipLaunchKernelGGL((k_enum_leaves_quads<false>), grid1, LEAF_THREADS, 0, s1, p->dev, pd, roots, b, e);
            else
                hipLaunchKernelGGL((k_enum_leaves<1, false>), grid1, LEAF_THREADS, 0, s1, p->dev, pd, roots, kChunk, b, e);
        }
        LP_HIP(ctx, hipEventRecord(ctx->aux_event[0], sT));
        LP_HIP(ctx, hipEventRecord(ctx->aux_event[2], s1));
        LP_HIP(ctx, hipStreamWaitEvent(s, ctx->aux_event[0], 0));
        LP_HIP(ctx, hipStreamWaitEvent(s, ctx->aux_event[2], 0));
        if (parent_tails) LP_HIP(ctx, hipStreamWaitEvent(s, ctx->aux_event[3], 0));   // k_enum_parent_tails, on its own stream
    } else {
        hipLaunchKernelGGL(k_enum_make_items<false>, lp_ceil_div(bound, 1024), 1024, 0, ctx->stream, p->dev, pd,
                           roots, level, bound, 0, 1, kChunk, 0, b, e);
        if (exact)
            hipLaunchKernelGGL((k_enum_leaves<0, true>), grid6, LEAF_THREADS, 0, ctx->stream, p->dev, pd, roots, kChunk, b, e);
        else
            hipLaunchKernelGGL((k_enum_leaves<0, false>), grid6, LEAF_THREADS, 0, ctx->stream, p->dev, pd, roots, kChunk, b, e);
    }
    return LP_OPTIMAL;
}

// ---- self-test of recip_midrange against the compiler's division (lp_debug_reciprocal) ----
namespace {
__global__ void k_debug_reciprocal(const double* __restrict__ x, int n, double* __restrict__ fast,
                                   double* __restrict__ plain) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = x[i];
    fast[i] = recip_midrange(v);
    asm volatile("" : "+v"(v));   // (two separate computations, whatever the optimiser thinks of them)
    plain[i] = 1.0 / v;
}
}  // namespace

int lp_enum_debug_reciprocal(lp_context* ctx, const double* x, int n, double* fast_out, double* plain_out) {
    double *dx = nullptr, *df = nullptr, *dp = nullptr;
    const size_t bytes = sizeof(double) * (size_t)n;
    LP_HIP(ctx, hipMalloc(&dx, bytes));
    hipError_t e = hipMalloc(&df, bytes);
    if (e == hipSuccess) e = hipMalloc(&dp, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(dx, x, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_reciprocal, (unsigned)lp_ceil_div(n, 256), 256, 0, ctx->stream, dx, n, df, dp);
        e = hipMemcpyAsync(fast_out, df, bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(plain_out, dp, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(dx);
    (void)hipFree(df);
    (void)hipFree(dp);
    LP_HIP(ctx, e);
    return LP_OPTIMAL;
}

#ifdef LP_LEAF_WAVELOG
// Diagnostic builds only (-DLP_LEAF_WAVELOG, scripts/leaf_wavelog.py): copies the wave log out (6 words per wave),
// returns the number of entries and empties the log.
extern "C" int lp_debug_leaf_wavelog(unsigned long long* out, int cap) {
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_wavelog_n), sizeof(n)) != hipSuccess) return -1;
    if (n > (unsigned)kWaveLogCap) n = kWaveLogCap;
    if ((int)n > cap) n = (unsigned)cap;
    if (out && n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wavelog), sizeof(unsigned long long) * 6 * n) != hipSuccess) return -1;
    const unsigned int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_wavelog_n), &zero, sizeof(zero)) != hipSuccess) return -1;
    return (int)n;
}
#endif
