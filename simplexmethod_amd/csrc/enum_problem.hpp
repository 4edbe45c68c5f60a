// enum_problem.hpp — device-side state of one vertex enumeration.
#pragma once

#include "lp_internal.hpp"

constexpr int kEnumMaxN = 64;   // ranks must fit u64: C(64,32) < 2^64
constexpr int kEnumMaxM = 32;
constexpr int kBinomK = kEnumMaxM + 2;  // columns of the binomial table

// Monotone double -> u64 key (so atomicMax on the key is max on the double).
__host__ __device__ inline unsigned long long lp_f64_key(double v) {
    unsigned long long b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = (unsigned long long)__double_as_longlong(v);
#else
    std::memcpy(&b, &v, sizeof(b));
#endif
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__host__ __device__ inline double lp_key_f64(unsigned long long k) {
    unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)b);
#else
    double v;
    std::memcpy(&v, &b, sizeof(v));
    return v;
#endif
}

// Results of one pass, accumulated with device-scope atomics.
struct EnumResult {
    unsigned long long best_key;    // key of the best score (score = z if maximize else -z)
    unsigned long long counts[3];   // feasible, infeasible, singular
    unsigned long long first_rank;  // pass 2: smallest qualifying rank
    unsigned long long range_flag;  // leaf kernels, fast reciprocal: some pivot left its range — the pass is repeated with plain divisions
    unsigned long long pad[2];
};

// What the host reads back after a shared-prefix pass, in ONE device block and one pinned mirror (one copy per
// pass instead of four: each small device-to-host copy is a 5-20 us blit on the stream, a tenth of the fixed cost
// of an 8-way shard).  EnumDev::result, PrefixDev::list_count / overflow / level_counts point into the device block.
struct EnumPassBlock {
    EnumResult result;
    unsigned long long list_count;
    int overflow;
    int pad;
    int level_counts[32];
};

struct EnumDev {
    int m, n, lda;                  // lda = n + 1 (odd stride: conflict-free row gathers)
    int maximize;
    int rs;                         // row stride of 32-row prefix records: m rounded up to even (enum_tree.hpp)
    int pad0;
    const double* A;                // m x lda row-major copy of the canonical A (pad column 0)
    const double* b;                // m
    const double* c;                // n
    const unsigned long long* binom;  // (kEnumMaxN+1) x kBinomK table, C(i,k)
    EnumResult* result;
    double* chunk_best;             // per-chunk best score of the last pass 1
};

// Shared-prefix path (enum_prefix.hip)
struct PrefixDev {
    int* level_counts;                // [32]: records of each tree level (level 0 = 1), device side
    int* overflow;                    // != 0: a buffer was too small, the caller falls back
    int* root_cursor;                 // [2] work cursors (regular / thin leaf kernel, sweep groups)
    unsigned long long* list;         // ranks of feasible subsets
    int* list_rec;                    // record (last breadth-first level) each entry was found under
    unsigned long long* list_count;
    unsigned long long list_cap;
    unsigned long long list_abort;    // leaf kernels stop drawing items once the list count exceeds this
    double* scores;                   // objective score of each list entry (after evaluation)
    double* dense_scores;             // dense form (degenerate LPs): score of every subset of the range, by
    unsigned long long dense_cap;     // rank - begin (-inf: not feasible); no list
    int4* items;                      // leaf-kernel work items, table 0: (record, child column, first subset, rank offset)
    int4* items2;                     // table 1 (two-level kernel): (record, child | j2 << 8, first subset, rank offset)
    int* item_count;                  // [2]
    int item_cap, item_cap2;
    const unsigned* comb4;            // same for 4-subsets (third level of the leaf kernel)
    const unsigned* comb5;            // same for 5-subsets (second level of the leaf kernel)
    const unsigned* comb6;            // [32 offsets][entries]: all 6-subsets of R columns in lex order,
                                      // 5 bits per index; entry of leaf l of R columns = comb6[comb6[R] + l]
};

// Test and A/B knobs of the enumeration, read from the environment once, by lp_enum_upload
// (enum_driver.hip: read_knobs), so that a problem's route cannot change between two calls.
struct EnumKnobs {
    unsigned long long list_cap = 1ULL << 22;  // first feasible-list capacity (LP_ENUM_LIST_CAP / LP_ENUM_LIST_START)
    bool list_pinned = false;        // LP_ENUM_LIST_CAP: the list neither grows nor gives way to the dense form
    size_t level_budget = SIZE_MAX;  // LP_ENUM_LEVEL_BUDGET_KB in bytes (SIZE_MAX: by device memory)
    bool exact_div = false;          // LP_ENUM_EXACT_DIV=1: plain divisions from the first pass on
    int narrow_mult = -1;            // LP_ENUM_NARROW_MULT (-1: by record width)
    int chunk1 = 0;                  // LP_ENUM_CHUNK: subsets per table-1 leaf item, a power of two from 1024 to 16384 (0: by range)
    int parent_tails = -1;           // LP_ENUM_PARENT_TAILS: 0 = every depth m-7 node is stored and finished from its own record,
                                     // 1 = the narrow ones from their parents' on any range (-1: by range size)
    int leaf_quads = -1;             // LP_ENUM_LEAF_QUADS: 0 = table 0 by k_enum_leaves<1> with paired items, 1 = by
                                     // k_enum_leaves_quads, one entry per child (-1: the default, the latter)
};

// The feasible list a successful shared-prefix pass left on the device (prefix.list / scores, or in the
// dense form prefix.dense_scores by rank - begin), and the tie rule the pass already applied to it.
struct EnumList {
    uint64_t begin = 0, end = 0;
    uint64_t n = 0;                  // feasible subsets
    bool dense = false;
    double star = 0.0, tol = 0.0;    // the tie rule applied: the list's own best score, Solver::EPS ...
    uint64_t first = ~0ULL;          // ... and its answer
};

// A range whose feasible subsets do not fit the list (degenerate LPs: up to every non-singular basis is
// feasible), or whose depth m-7 nodes do not fit the level buffers, is enumerated in sub-ranges, one
// list at a time; pass 2 re-runs only the sub-ranges whose best score can hold the winner.
struct EnumSubRange {
    uint64_t begin, end;
    double best;     // best score of the sub-range (-inf: no feasible subset)
    bool direct;     // the sub-range ran on the direct kernel (no list)
};

// What the last lp_enum_range left for pass 2 over the same range: written by lp_enum_range only,
// read by lp_enum_first_within only.
struct EnumRangeRecord {
    enum Kind { kNone, kList, kSubRanges } kind = kNone;   // kNone: pass 2 runs the direct kernel
    uint64_t begin = 0, end = 0;
    EnumList list;                   // kList
    std::vector<EnumSubRange> parts; // kSubRanges, ascending
};

struct lp_enum_problem {
    lp_context* ctx = nullptr;
    bool complete = false;           // every allocation of lp_enum_upload succeeded (a shell worth keeping)
    EnumKnobs knobs;
    EnumDev dev{};
    double* dA = nullptr;
    double* db = nullptr;
    double* dc = nullptr;
    unsigned long long* dbinom = nullptr;
    EnumPassBlock* d_pass = nullptr; // the device block behind dev.result, prefix.list_count / overflow / level_counts
    EnumPassBlock* h_pass = nullptr; // pinned mirror; the four h_* pointers below point into it
    EnumResult* h_result = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the last direct launch of pass 1 (enum_direct.hip): how its per-chunk best scores lie in
    // dev.chunk_best, so that pass 2 over the same range narrows to the first qualifying chunk
    struct DirectLaunch {
        uint64_t begin = 0, end = 0, per_chunk = 0;
        int chunks = 0;
    } last_direct;
    int chunk_cap = 0;
    std::vector<double> h_chunk_best;
    // vertex scratch
    double* dvx = nullptr;  // kEnumMaxM xB values + 1 objective
    int* dvi = nullptr;     // kEnumMaxM subset + 1 verdict
    // shared-prefix path
    PrefixDev prefix{};
    double* prefix_buf[2] = {nullptr, nullptr};
    size_t prefix_buf_bytes[2] = {0, 0};
    int* h_level_counts = nullptr;             // pinned copy of the 32 level counts
    unsigned long long* h_list_count = nullptr;  // pinned
    int* h_overflow = nullptr;                 // pinned
    uint64_t split_hint = 0;
    // dense_hint: a pass found more than a third of its range feasible; later passes of this problem
    // start in the dense form (enum_driver.hip: enum_prefix_pass)
    bool dense_hint = false;
    // the leaf kernels divide plainly (enum_leaf.hip: leaf_verdict): set for good once a pass of the fast
    // kernels met pivots outside the fast reciprocal's exponent range, or by LP_ENUM_EXACT_DIV=1 (A/B, tests)
    bool exact_div = false;
    EnumRangeRecord last_range;
    // shard of the last lp_enum_solve_sharded call (enum_sharded.hip)
    int shard_rank = -1, shard_world = -1;
    uint64_t shard_lo = 0, shard_hi = 0;
};

// enum_driver.hip: releases the enumeration shells the context keeps (lp_context_destroy)
void lp_enum_release_shells(lp_context* ctx);

// enum_direct.hip
int lp_enum_direct_range(lp_enum_problem* p, uint64_t begin, uint64_t end, double* score_best,
                         uint64_t counts[3], lp_enum_stats* stats);
int lp_enum_direct_first(lp_enum_problem* p, uint64_t begin, uint64_t end, double score_star,
                         double tol, uint64_t* rank_out);
int lp_enum_direct_vertex(lp_enum_problem* p, uint64_t rank, double* xB, int* subset, double* z,
                          int* verdict);
// smallest rank of the list whose score is within tol of score_star (UINT64_MAX if none)
int lp_enum_list_first(lp_enum_problem* p, const EnumList& list, double score_star, double tol, uint64_t* rank_out);
// evaluation + tie rule against the list's own best, queued without a host round trip; records !=
// null: the depth m-7 records of the pass (the entries are evaluated from them, enum_leaf.hip); no_record: some entries
// have none (list_rec = -1, k_enum_parent_tails) and are solved from scratch beside them
int lp_enum_queue_list_tail(lp_enum_problem* p, double tol, const double* records, bool no_record);
int lp_enum_queue_dense_tail(lp_enum_problem* p, double tol, uint64_t begin, uint64_t end);
void lp_enum_queue_record_eval(lp_enum_problem* p, const double* records);

// enum_prefix.hip: the root record (pg = 16 or 32 rows; also resets the pass's counters), and level t -> t+1
// of the breadth-first phase (bound: the level's parents inside [begin, end); narrow: one wave per child)
void lp_enum_launch_root(lp_enum_problem* p, int pg, double* dst);
// stop: the first column whose child is not expanded (n: every child is)
void lp_enum_launch_level(lp_enum_problem* p, int shape, int t, bool narrow, uint64_t bound, const double* src,
                          int src_cap, double* dst, int cap, int stop, uint64_t begin, uint64_t end);

// enum_leaf.hip: one lane per subset below the records of the last breadth-first level
// (shape: enum_driver.hip: prefix_shape — 1 = the tuned kernels, 2 / 3 = the general kernel on 16- / 32-row records)
// dense: every subset's score goes to prefix.dense_scores[rank - begin] (general kernel), no list
// parent_tails: lp_enum_launch_parent_tails was queued for this pass (the library's stream joins it at the end)
int lp_enum_launch_leaves(lp_enum_problem* p, const double* roots, int bound, int level, bool fused,
                          int shape, bool dense, bool parent_tails, uint64_t begin, uint64_t end);
// enum_leaf.hip: whether this pass finishes its narrow depth m-7 nodes from the depth m-8 records (the tuned leaf
// kernels only: shape 1, fused, list form, at least one level; records: the depth m-7 nodes of the range), and the
// first column of such a node (n - 1 - THIN_TAIL)
bool lp_enum_parent_tails(const lp_enum_problem* p, int shape, bool fused, bool dense, int level, uint64_t records);
int lp_enum_parent_tails_stop(int n);
// ... and the kernel that finishes them from the depth m-8 records (`bound` of them at most, level = m-8), on the tail
// kernel's stream behind what the library's stream holds when it is called
int lp_enum_launch_parent_tails(lp_enum_problem* p, const double* parents, int bound, int level, uint64_t begin,
                                uint64_t end);
// enum_leaf.hip: recip_midrange(x[i]) and 1.0 / x[i] computed on the device (lp_debug_reciprocal)
int lp_enum_debug_reciprocal(lp_context* ctx, const double* x, int n, double* fast_out, double* plain_out);
