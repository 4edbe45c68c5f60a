// enum_driver.hip — the host side of the vertex enumeration: its C ABI (lp_enum_*) and every decision a
// range pass makes: the shared-prefix path or the direct kernel, the feasible list's size and growth, the
// dense form, sub-ranges, and pass 2 (the tie rule).  The kernel files launch (enum_prefix.hip: root and
// levels, enum_leaf.hip: leaves, enum_direct.hip: the direct kernel and the lists' tails); this file decides.
#include <cmath>
#include <cstdlib>
#include <memory>

#include "enum_problem.hpp"
#include "enum_tree.hpp"

using lptree::NMX;
using lptree::PG;

// Private outcomes of the shared-prefix path; none of them ever leaves an lp_* function.
// kEnumNoRoom: no memory for the level buffers, or a level outgrew its buffer (the device's overflow flag):
// the direct kernel enumerates the range
constexpr int kEnumNoRoom = 1000;
// kEnumListOverflow: the feasible list was too small; *h_list_count holds the number of feasible subsets
// of the range, the caller grows the list, goes dense or splits the range
constexpr int kEnumListOverflow = 1001;
// kEnumRangeTooWide: the range has more depth m-7 nodes than the level buffers hold; the caller splits it
// into about p->split_hint parts
constexpr int kEnumRangeTooWide = 1002;

// the shared-prefix path cannot take this range as it is: the direct kernel does
static bool go_direct(int rc) { return rc == kEnumNoRoom || rc == kEnumListOverflow || rc == kEnumRangeTooWide; }

static EnumKnobs read_knobs() {
    EnumKnobs k;
    if (const char* e = getenv("LP_ENUM_LIST_CAP")) {   // tests: force the sub-range path on small problems
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 64 && v < k.list_cap) k.list_cap = v;
        k.list_pinned = true;
    } else if (const char* e2 = getenv("LP_ENUM_LIST_START")) {   // tests: a small first list that may grow
        const unsigned long long v = strtoull(e2, nullptr, 10);
        if (v >= 64 && v < k.list_cap) k.list_cap = v;
    }
    if (const char* e = getenv("LP_ENUM_LEVEL_BUDGET_KB")) k.level_budget = (size_t)strtoull(e, nullptr, 10) << 10;
    if (const char* e = getenv("LP_ENUM_EXACT_DIV")) k.exact_div = atoi(e) != 0;
    if (const char* e = getenv("LP_ENUM_NARROW_MULT")) k.narrow_mult = atoi(e);
    if (const char* e = getenv("LP_ENUM_CHUNK")) {
        const int v = atoi(e);
        if (v >= 1024 && v <= 16384 && (v & (v - 1)) == 0) k.chunk1 = v;
    }
    if (const char* e = getenv("LP_ENUM_PARENT_TAILS")) k.parent_tails = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("LP_ENUM_LEAF_QUADS")) k.leaf_quads = atoi(e) != 0 ? 1 : 0;
    return k;
}

// ---------------------------------------------------------------------------
// combinatorics of the rank space
// ---------------------------------------------------------------------------

static size_t host_rec_doubles(int n, int t, int pg, int rs) {
    return (size_t)(pg == 32 ? rs : pg) * (n - t + 1) + (pg == 32 ? 12 : 8);
}

// Number of depth-t tree nodes whose subtree meets the rank range [begin, end): the length-t
// prefixes of the subsets begin .. end-1 are consecutive in the lexicographic order of the
// t-subsets of {0 .. n-m+t-1}, so the count is the difference of two prefix ranks, plus one.
uint64_t lp_host_prefix_rank(int n, int m, uint64_t rank, int t) {
    // unrank the first t elements of the rank-th m-subset, accumulating their rank among t-subsets
    uint64_t pr = 0;
    int a = 0;
    for (int k = 0; k < t; ++k) {
        int j = a;
        for (;; ++j) {
            const uint64_t cnt = lp_host_binom(n - 1 - j, m - 1 - k);
            if (rank < cnt) break;
            rank -= cnt;
            pr += lp_host_binom(n - m + t - 1 - j, t - 1 - k);  // t-prefixes starting ..j.. lie before
        }
        a = j + 1;
    }
    return pr;
}
static uint64_t host_level_nodes(int n, int m, uint64_t begin, uint64_t end, int t) {
    if (end <= begin) return 0;
    return lp_host_prefix_rank(n, m, end - 1, t) - lp_host_prefix_rank(n, m, begin, t) + 1;
}

// Every k-subset of R = k .. rmax columns in lexicographic order, 5 bits per index: entry l of R
// columns = table[table[R] + l] (the leaf kernels' subset tables, shape-independent)
static std::vector<unsigned> subset_table(int k, int rmax) {
    std::vector<unsigned> table(32, 0u);
    for (int R = k; R <= rmax; ++R) {
        table[(size_t)R] = (unsigned)table.size();
        int s[6];
        for (int t = 0; t < k; ++t) s[t] = t;
        for (;;) {
            unsigned pk = 0;
            for (int t = 0; t < k; ++t) pk |= (unsigned)s[t] << (5 * t);
            table.push_back(pk);
            int t = k - 1;
            while (t >= 0 && s[t] == R - k + t) --t;
            if (t < 0) break;
            ++s[t];
            for (int u = t + 1; u < k; ++u) s[u] = s[u - 1] + 1;
        }
    }
    return table;
}

// Shapes of the shared-prefix path:
//   1  m in 6..16, n-m in 2..16: 16-row records, the tuned leaf kernels (subset tables, LDS slices)
//   2  m in 7..16, n-m in 17..57 (n <= 64): 16-row records, the general leaf kernel
//   3  m in 17..32, n-m in 2..32: 32-row records, the general leaf kernel
//   0  everything else (direct kernel)
static int prefix_shape(const lp_enum_problem* p) {
    const int m = p->dev.m, nm = p->dev.n - p->dev.m;
    if (nm < 2) return 0;
    if (m >= 6 && m <= PG && nm <= NMX) return 1;
    if (m >= 7 && m <= PG && nm <= 57) return 2;
    if (m > PG && m <= 32 && nm <= 32) return 3;
    return 0;
}

// ---------------------------------------------------------------------------
// problem state: the feasible list, the kept shells
// ---------------------------------------------------------------------------

// The feasible list of the shared-prefix path: rank, record index and score of each entry.
static void enum_list_release(lp_enum_problem* p) {
    PrefixDev& pd = p->prefix;
    lp_pool_release(p->ctx, pd.list, sizeof(unsigned long long) * pd.list_cap);
    lp_pool_release(p->ctx, pd.scores, sizeof(double) * pd.list_cap);
    lp_pool_release(p->ctx, pd.list_rec, sizeof(int) * pd.list_cap);
    pd.list = nullptr;
    pd.scores = nullptr;
    pd.list_rec = nullptr;
    pd.list_cap = 0;
}
static hipError_t enum_list_alloc(lp_enum_problem* p, unsigned long long cap) {
    PrefixDev& pd = p->prefix;
    size_t got = 0;
    hipError_t e = lp_pool_alloc(p->ctx, (void**)&pd.list, sizeof(unsigned long long) * cap, &got);
    if (e == hipSuccess) e = lp_pool_alloc(p->ctx, (void**)&pd.scores, sizeof(double) * cap, &got);
    if (e == hipSuccess) e = lp_pool_alloc(p->ctx, (void**)&pd.list_rec, sizeof(int) * cap, &got);
    if (e != hipSuccess) {
        // the sizes lp_pool_release is told must be those of the failed request
        pd.list_cap = cap;
        enum_list_release(p);
        return e;
    }
    pd.list_cap = cap;
    return hipSuccess;
}

// Makes the feasible list hold `nfeas` entries (20 bytes each) if the device has the memory.
static bool enum_list_grow(lp_enum_problem* p, uint64_t nfeas) {
    if (p->knobs.list_pinned) return false;
    const unsigned long long old_cap = p->prefix.list_cap;
    const unsigned long long want = nfeas + nfeas / 16 + 4096;
    if (want <= old_cap) return false;
    (void)hipSetDevice(p->ctx->device);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    if ((size_t)want * 20 + (size_t(2) << 30) > free_b) return false;
    enum_list_release(p);
    if (enum_list_alloc(p, want) == hipSuccess) return true;
    (void)hipGetLastError();
    if (enum_list_alloc(p, old_cap) != hipSuccess) p->complete = false;   // (cannot happen: it was just released)
    return false;
}

static void enum_destroy(lp_enum_problem* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipFree(p->dA); (void)hipFree(p->db); (void)hipFree(p->dc); (void)hipFree(p->dbinom);
    (void)hipFree(p->d_pass); (void)hipFree(p->dev.chunk_best);
    (void)hipFree(p->dvx); (void)hipFree(p->dvi);
    (void)hipFree(p->prefix.root_cursor);
    enum_list_release(p);
    lp_pool_release(p->ctx, p->prefix.dense_scores, sizeof(double) * p->prefix.dense_cap);
    lp_pool_release(p->ctx, p->prefix.items, sizeof(int4) * (size_t)p->prefix.item_cap);
    lp_pool_release(p->ctx, p->prefix.items2, sizeof(int4) * (size_t)p->prefix.item_cap2);
    (void)hipFree(p->prefix.item_count);
    lp_pool_release(p->ctx, p->prefix_buf[0], p->prefix_buf_bytes[0]);
    lp_pool_release(p->ctx, p->prefix_buf[1], p->prefix_buf_bytes[1]);
    if (p->h_pass) (void)hipHostFree(p->h_pass);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    delete p;
}

void lp_enum_release_shells(lp_context* ctx) {
    for (void* q : ctx->enum_shells) enum_destroy(static_cast<lp_enum_problem*>(q));
    ctx->enum_shells.clear();
}

// ---------------------------------------------------------------------------
// one shared-prefix pass
// ---------------------------------------------------------------------------

static int prefix_range_once(lp_enum_problem* p, uint64_t begin, uint64_t end, double* score_best,
                             uint64_t counts[3], lp_enum_stats* stats, bool dense, EnumList* list) {
    lp_context* ctx = p->ctx;
    const EnumDev& d = p->dev;
    hipStream_t s = ctx->stream;
    const int m = d.m, n = d.n;
    const int shape = prefix_shape(p);
    const int pg = shape == 3 ? 32 : PG;
    // breadth-first to depth m-7 (m-6 for m = 6), then one lane per subset (enum_leaf.hip)
    // (the leaf kernel performs the pivot of depth m-6 itself, so the levels stop at depth m-7)
    const bool fused = m >= 7;
    const int D0 = fused ? m - 7 : m - 6;
    PrefixDev& pd = p->prefix;
    if (dense && !fused) dense = false;
    // a listing pass whose list is already 16x over capacity stops early: the caller goes dense on that
    // count alone (LP_ENUM_LIST_CAP, the tests' pinned list, needs the exact count for its sub-ranges)
    pd.list_abort = (fused && !p->knobs.list_pinned) ? 16 * pd.list_cap : ~0ULL;
    if (dense && pd.dense_cap < end - begin) {   // rank-indexed scores of the range (8 bytes per subset)
        lp_pool_release(ctx, pd.dense_scores, sizeof(double) * pd.dense_cap);
        pd.dense_scores = nullptr;
        pd.dense_cap = 0;
        size_t got = 0;
        if (lp_pool_alloc(ctx, (void**)&pd.dense_scores, sizeof(double) * (end - begin), &got) == hipSuccess) {
            pd.dense_cap = got / sizeof(double);
        } else {
            (void)hipGetLastError();
            dense = false;   // no memory for it: the list form
        }
    }
    // ---- buffers: two ping-pong level arrays sized for the widest level (depth D0) of the whole
    // problem if that fits the budget (C(32,16): 6.4 GB), otherwise for as many records as fit; a
    // range with more depth-D0 nodes than that is split by the caller (kEnumRangeTooWide)
    const uint64_t nodes_max = lp_host_binom(n - m + D0, D0);
    const uint64_t nodes_prev = D0 >= 1 ? lp_host_binom(n - m + D0 - 1, D0 - 1) : 1;
    const size_t rec_bytes = host_rec_doubles(n, D0, pg, d.rs) * sizeof(double);
    const size_t rec_prev_bytes = host_rec_doubles(n, D0 >= 1 ? D0 - 1 : 0, pg, d.rs) * sizeof(double);
    uint64_t cap_budget0 = 0, cap_budget1 = 0;   // records the budget allows at depth D0 / D0-1
    {
        if (ctx->total_mem == 0) {
            size_t free_b = 0;
            LP_HIP(ctx, hipMemGetInfo(&free_b, &ctx->total_mem));
        }
        size_t budget = std::min<size_t>(ctx->total_mem / 5 * 2, size_t(24) << 30);   // for both buffers together
        if (p->knobs.level_budget != SIZE_MAX) budget = p->knobs.level_budget;
        // level D0-1 holds at most as many records as level D0 (every record has a child or is a hole)
        const uint64_t cap0 = std::max<uint64_t>(std::min<uint64_t>(nodes_max, budget / (rec_bytes + rec_prev_bytes)), 1);
        const uint64_t cap1 = std::min<uint64_t>(nodes_prev, cap0);
        cap_budget0 = cap0;
        cap_budget1 = cap1;
        const size_t want[2] = {(size_t)cap0 * rec_bytes, std::max<size_t>((size_t)cap1 * rec_prev_bytes, 4096)};
        for (int k = 0; k < 2; ++k) {
            if (p->prefix_buf_bytes[k] >= want[k]) continue;
            lp_pool_release(ctx, p->prefix_buf[k], p->prefix_buf_bytes[k]);
            p->prefix_buf[k] = nullptr;
            p->prefix_buf_bytes[k] = 0;
            size_t got = 0;
            hipError_t e = lp_pool_alloc(ctx, (void**)&p->prefix_buf[k], want[k], &got);
            if (e != hipSuccess) {
                // give back what the context's pool holds before giving up on this path
                (void)hipGetLastError();
                for (auto& blk : ctx->pool) (void)hipFree(blk.first);
                ctx->pool.clear();
                e = lp_pool_alloc(ctx, (void**)&p->prefix_buf[k], want[k], &got);
            }
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return kEnumNoRoom;
            }
            p->prefix_buf_bytes[k] = got;
        }
    }
    uint64_t nodes_d0 = 0;   // depth-D0 nodes of the range
    {
        // the range's own node counts (exact) against what the buffers hold
        // (a kept buffer may be larger than this problem's budget share: the budget decides, so that the
        // behaviour does not depend on what ran before)
        const uint64_t have0 = std::min<uint64_t>(p->prefix_buf_bytes[0] / rec_bytes, cap_budget0);
        const uint64_t have1 = std::min<uint64_t>(p->prefix_buf_bytes[1] / rec_prev_bytes, cap_budget1);
        const uint64_t want0 = nodes_d0 = host_level_nodes(n, m, begin, end, D0);
        const uint64_t want1 = D0 >= 1 ? host_level_nodes(n, m, begin, end, D0 - 1) : 1;
        if (want0 > have0 || want1 > have1 || want0 > 0x7FFFFFFFULL) {
            p->split_hint = std::max<uint64_t>(want0 / std::max<uint64_t>(have0, 1), want1 / std::max<uint64_t>(have1, 1)) + 1;
            return kEnumRangeTooWide;
        }
    }
    // depth-D0 records always end in buffer 0; levels alternate so that level D0 lands there
    LP_HIP(ctx, hipEventRecord(p->ev0, s));
    // dense form: only subsets under live depth-D0 records get a score from the leaf kernel; subtrees
    // pruned as singular leave their entries untouched, and the tie rule scans the whole range.  All
    // bits set = NaN, which fails its `>=` test (the buffer comes from a pool: old scores, level records)
    if (dense) LP_HIP(ctx, hipMemsetAsync(pd.dense_scores, 0xFF, sizeof(double) * (end - begin), s));
    int launches = 0;
    // the narrow depth m-7 nodes (at most THIN_TAIL selectable columns) are finished from their parents' records
    // (enum_leaf.hip: k_enum_parent_tails) where the tuned leaf kernels run: the last level does not store them
    const bool parent_tails = lp_enum_parent_tails(p, shape, fused, dense, D0, nodes_d0);
    int cur = (D0 % 2 == 0) ? 0 : 1;  // buffer of level 0, so that level D0 is buffer 0
    // All levels and the leaf kernel are queued without a host round trip: every level's record
    // count stays on the device (level_counts[t]); grids are sized for the exact number of the
    // level's parents inside the range (blocks beyond the actual count return at once).
    lp_enum_launch_root(p, pg, p->prefix_buf[cur]);   // + all counters reset
    ++launches;
    int caps[32];
    caps[0] = 1;
    for (int t = 0; t < D0; ++t) {
        const int nxt = cur ^ 1;
        const uint64_t cap64 = p->prefix_buf_bytes[nxt] / (host_rec_doubles(n, t + 1, pg, d.rs) * sizeof(double));
        const int cap = cap64 > 0x7FFFFFFFULL ? 0x7FFFFFFF : (int)cap64;
        caps[t + 1] = cap;
        // parents of this level inside the range (exact; the level's holes are among them)
        const uint64_t bound = std::min<uint64_t>(host_level_nodes(n, m, begin, end, t), 0x7FFFFFFFULL);
        // narrow levels: one wave per (parent, child)
        // (every child of a narrow level takes its slot with a returning atomic of its own, ~11 ns each on the one
        // counter: beyond a few thousand candidate waves the per-parent kernels, one allocation per block, are faster —
        // 16-row records: the LDS-staged kernel expands the 969 parents of C(32,16)'s level 3 in a fraction of the
        // 61 us the narrow form took for their 4845 children)
        const uint64_t waves = bound * (uint64_t)(n - m + 1);
        const int narrow_mult = p->knobs.narrow_mult >= 0 ? p->knobs.narrow_mult : (pg == 16 ? 16 : 128);
        const bool narrow = waves <= (uint64_t)ctx->num_cus * (uint64_t)narrow_mult;
        const bool last_level = t == D0 - 1;
        const int stop = (parent_tails && last_level) ? lp_enum_parent_tails_stop(n) : n;
        if (parent_tails && last_level) {   // beside the last level, not behind it (measured: lp_enum_launch_parent_tails)
            const int rc = lp_enum_launch_parent_tails(p, p->prefix_buf[cur], (int)std::min<uint64_t>(bound, (uint64_t)caps[t]), t, begin, end);
            if (rc) return rc;
            ++launches;
        }
        lp_enum_launch_level(p, shape, t, narrow, bound, p->prefix_buf[cur], t == 0 ? 1 : caps[t], p->prefix_buf[nxt],
                             cap, stop, begin, end);
        ++launches;
        cur = nxt;
    }
    const uint64_t root_bound = std::min<uint64_t>(nodes_d0, 0x7FFFFFFFULL);
    {
        const int rc = lp_enum_launch_leaves(p, p->prefix_buf[cur], (int)std::min<uint64_t>(root_bound, (uint64_t)caps[D0]),
                                             D0, fused, shape, dense, parent_tails, begin, end);
        if (rc) {   // (no memory for an item table: nothing joined k_enum_parent_tails' stream)
            if (parent_tails) (void)hipStreamSynchronize(ctx->aux_stream[2]);
            return rc;
        }
    }
    ++launches;
    // objectives of the (few) feasible subsets by the direct solver, and the tie rule against this
    // range's own best score (what a sharded run asks next): queued behind the leaf kernels
    constexpr double kSpecTol = 1e-9;   // Solver::EPS, the tolerance dist.py / EnumerationSolver use
    if (dense)
        lp_enum_queue_dense_tail(p, kSpecTol, begin, end);
    else
        lp_enum_queue_list_tail(p, kSpecTol, fused ? p->prefix_buf[cur] : nullptr, parent_tails);
    LP_HIP(ctx, hipEventRecord(p->ev1, s));
    // result, list count, overflow flag and level counts: one block, one copy (enum_problem.hpp: EnumPassBlock)
    LP_HIP(ctx, hipMemcpyAsync(p->h_pass, p->d_pass, sizeof(EnumPassBlock), hipMemcpyDeviceToHost, s));
    LP_HIP(ctx, hipStreamSynchronize(s));
    LP_HIP(ctx, hipGetLastError());
    for (int t = 1; t <= D0; ++t)
        if (p->h_level_counts[t] > caps[t]) return kEnumNoRoom;  // a level buffer was too small
    if (*p->h_overflow != 0) return kEnumNoRoom;
    float ms = 0.f;
    LP_HIP(ctx, hipEventElapsedTime(&ms, p->ev0, p->ev1));
    if (!dense && *p->h_list_count > pd.list_cap) {   // the caller grows the list or splits the range
        if (stats) {
            stats->kernel_ms = ms;
            stats->subsets = end - begin;
            stats->launches = launches;
        }
        return kEnumListOverflow;
    }
    const uint64_t nfeas = dense ? p->h_result->counts[0] : *p->h_list_count;
    const double best = nfeas ? lp_key_f64(p->h_result->best_key) : -INFINITY;
    *list = {begin, end, nfeas, dense, best, kSpecTol, nfeas ? p->h_result->first_rank : ~0ULL};
    *score_best = best;
    for (int k = 0; k < 3; ++k) counts[k] = p->h_result->counts[k];
    if (stats) {
        stats->kernel_ms = ms;
        stats->subsets = end - begin;
        stats->launches = launches;
    }
    return LP_OPTIMAL;
}

// The leaf kernels run with the fast reciprocal (enum_leaf.hip: recip_midrange) until a pass reports a
// pivot outside its exponent range on a subset that is not singular anyway; that pass is repeated with
// plain divisions, and so is every later pass of the problem.
static int prefix_range(lp_enum_problem* p, uint64_t begin, uint64_t end, double* score_best, uint64_t counts[3],
                        lp_enum_stats* stats, bool dense, EnumList* list) {
    if (p->knobs.exact_div) p->exact_div = true;
    p->h_result->range_flag = 0ULL;
    int rc = prefix_range_once(p, begin, end, score_best, counts, stats, dense, list);
    if (!p->exact_div && p->h_result->range_flag != 0ULL) {
        p->exact_div = true;
        lp_enum_stats first{};
        if (stats) first = *stats;
        rc = prefix_range_once(p, begin, end, score_best, counts, stats, dense, list);
        if (stats) {
            stats->kernel_ms += first.kernel_ms;
            stats->launches += first.launches;
        }
    }
    return rc;
}

// One shared-prefix pass over [begin, end); on success *list describes the feasible list it left.  A list
// that overflows (a degenerate LP: up to every non-singular basis is feasible) either gives way to the
// dense form (a large part of the range feasible) or is re-allocated for the count the pass reported, if
// the device has the memory, and the pass runs once more.
static int enum_prefix_pass(lp_enum_problem* p, uint64_t begin, uint64_t end, double* score, uint64_t counts[3],
                            lp_enum_stats* stats, EnumList* list) {
    const bool may_dense = p->dev.m >= 7 && !p->knobs.list_pinned;
    auto again = [&](bool dense) {   // one more pass, times and launches added up
        lp_enum_stats first{};
        if (stats) first = *stats;
        const int rc = prefix_range(p, begin, end, score, counts, stats, dense, list);
        if (stats) {
            stats->kernel_ms += first.kernel_ms;
            stats->launches += first.launches;
        }
        return rc;
    };
    int rc = prefix_range(p, begin, end, score, counts, stats, p->dense_hint && may_dense, list);
    if (rc == LP_OPTIMAL && list->dense) {
        if (counts[0] * 8 < end - begin) p->dense_hint = false;   // not that degenerate after all
        return rc;
    }
    if (rc == kEnumListOverflow && may_dense &&
        (*p->h_list_count > p->prefix.list_abort || *p->h_list_count * 3 > end - begin)) {
        // more than a third of the range is feasible (the pass reported the count), or the pass stopped
        // early on a list 16x over capacity: the dense form — no list, every subset's score by rank —
        // and later passes of this problem start there
        p->dense_hint = true;
        rc = again(true);
        if (rc == LP_OPTIMAL && list->dense) return rc;
    }
    if (rc == kEnumListOverflow && enum_list_grow(p, *p->h_list_count)) rc = again(false);
    return rc;
}

// Shared-prefix enumeration of a range in sub-ranges: because its depth m-7 nodes do not fit the level
// buffers (large shapes: C(n-7, m-7) records), or because its feasible subsets overflow a list that
// cannot grow.  A sub-range that still does not fit is split again.  Counts add, the best score is
// the maximum; every sub-range keeps its best score for pass 2 (*parts, ascending).
static int enum_prefix_chunked(lp_enum_problem* p, uint64_t begin, uint64_t end, uint64_t parts0,
                               double* score_best, uint64_t counts[3], lp_enum_stats* stats,
                               std::vector<EnumSubRange>* parts) {
    parts->clear();
    struct Part { uint64_t b, e; };
    std::vector<Part> todo;
    auto split = [&](uint64_t b, uint64_t e, uint64_t n) {   // pushes in DEscending order (stack)
        if (n < 2) n = 2;
        if (n > e - b) n = e - b;
        for (uint64_t k = n; k-- > 0;) {
            const uint64_t pb = b + (e - b) / n * k + std::min<uint64_t>(k, (e - b) % n);
            const uint64_t pe = b + (e - b) / n * (k + 1) + std::min<uint64_t>(k + 1, (e - b) % n);
            todo.push_back({pb, pe});
        }
    };
    split(begin, end, parts0);
    double best = -INFINITY;
    float ms = 0.f;
    int launches = 0;
    for (int k = 0; k < 3; ++k) counts[k] = 0;
    while (!todo.empty()) {
        const Part part = todo.back();
        todo.pop_back();
        double sc = -INFINITY;
        uint64_t cn[3] = {0, 0, 0};
        lp_enum_stats st{};
        EnumList list;
        int rc = enum_prefix_pass(p, part.b, part.e, &sc, cn, &st, &list);
        if (rc == kEnumListOverflow && part.e - part.b > 1 && *p->h_list_count * 2 <= part.e - part.b) {
            split(part.b, part.e, *p->h_list_count / (p->prefix.list_cap / 2) + 1);
            continue;
        }
        if (rc == kEnumRangeTooWide && part.e - part.b > 1) {
            split(part.b, part.e, p->split_hint + 1);
            continue;
        }
        const bool direct = go_direct(rc);
        if (direct) rc = lp_enum_direct_range(p, part.b, part.e, &sc, cn, &st);
        if (rc) return rc;
        parts->push_back({part.b, part.e, sc, direct});
        if (sc > best) best = sc;
        for (int k = 0; k < 3; ++k) counts[k] += cn[k];
        ms += st.kernel_ms;
        launches += st.launches;
    }
    *score_best = best;
    if (stats) {
        stats->kernel_ms = ms;
        stats->subsets = end - begin;
        stats->launches = launches;
    }
    return LP_OPTIMAL;
}

static int check_range(lp_enum_problem* p, uint64_t begin, uint64_t end) {
    const uint64_t total = lp_host_binom(p->dev.n, p->dev.m);
    if (begin > end || end > total) LP_FAIL(p->ctx, LP_BAD_ARG, "rank range outside [0, C(n,m)]");
    return LP_OPTIMAL;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" {

uint64_t lp_binom(int n, int k) { return lp_host_binom(n, k); }

// Cost-balanced cut of the rank space (same rule as simplexmethod_amd/dist.py:
// balanced_shard_bounds): cost(x) = x + kShardRecordCost * (depth m-7 tree nodes before subset x).
static const uint64_t kShardRecordCost = 160;
int lp_enum_shard_bounds(int n, int m, int shard, int shards, uint64_t* begin_out, uint64_t* end_out) {
    if (!begin_out || !end_out || shards <= 0 || shard < 0 || shard >= shards) return LP_BAD_ARG;
    if (m <= 0 || n < m || n > kEnumMaxN || m > kEnumMaxM) return LP_BAD_ARG;
    const uint64_t total = lp_host_binom(n, m);
    if (total == 0) return LP_BAD_ARG;
    const int d0 = m - 7;
    // (the cost model is that of the tuned kernels' box; the general kernel's shapes — m > 16 or
    // n - m > 16 — small trees and the direct kernel get equal-size cuts)
    const bool tuned_shape = m >= 7 && m <= 16 && n - m >= 2 && n - m <= 16;
    if (shards == 1 || !tuned_shape || total < (1ULL << 20)) {
        // (dist.py uses total * k // world here; same partition property, sizes differ by <= 1)
        *begin_out = (uint64_t)((unsigned __int128)total * (unsigned)shard / (unsigned)shards);
        *end_out = (uint64_t)((unsigned __int128)total * (unsigned)(shard + 1) / (unsigned)shards);
        return LP_OPTIMAL;
    }
    auto cost = [&](uint64_t x) -> unsigned __int128 {
        if (x >= total) return (unsigned __int128)total + (unsigned __int128)kShardRecordCost * lp_host_binom(n - 7, d0);
        return (unsigned __int128)x + (unsigned __int128)kShardRecordCost * lp_host_prefix_rank(n, m, x, d0);
    };
    const unsigned __int128 full = cost(total);
    auto cut = [&](int k) -> uint64_t {
        if (k <= 0) return 0;
        if (k >= shards) return total;
        const unsigned __int128 target = full * (unsigned)k / (unsigned)shards;
        uint64_t lo = 0, hi = total;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (cost(mid) < target) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    *begin_out = cut(shard);
    *end_out = cut(shard + 1);
    return LP_OPTIMAL;
}

int lp_enum_exact_division(const lp_enum_problem* p) { return (p && p->exact_div) ? 1 : 0; }

// A freed problem keeps its allocations (all sized for the largest shape) in the context for the next
// lp_enum_upload; beyond two kept shells it is really released.
void lp_enum_free(lp_enum_problem* p) {
    if (!p) return;
    lp_context* ctx = p->ctx;
    if (p->complete && ctx->enum_shells.size() < 2) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        ctx->enum_shells.push_back(p);
        return;
    }
    enum_destroy(p);
}

int lp_enum_upload(lp_context* ctx, const double* A, int m, int n, const double* b,
                   const double* c, int maximize, lp_enum_problem** problem_out) {
    if (!ctx || !problem_out) return LP_BAD_ARG;
    *problem_out = nullptr;
    if (!A || !b || !c) LP_FAIL(ctx, LP_BAD_ARG, "null problem array");
    if (m <= 0 || n < m) LP_FAIL(ctx, LP_BAD_ARG, "need 0 < m <= n");
    if (n > kEnumMaxN || m > kEnumMaxM)
        LP_FAIL(ctx, LP_BAD_ARG, "enumeration supports n <= 64 and m <= 32 (ranks must fit 64 bits)");
    if (lp_host_binom(n, m) == 0) LP_FAIL(ctx, LP_BAD_ARG, "C(n,m) overflows 64 bits");
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const EnumKnobs knobs = read_knobs();
    lp_enum_problem* p = nullptr;
    while (!p && !ctx->enum_shells.empty()) {   // a kept shell: every allocation is already there
        lp_enum_problem* q = static_cast<lp_enum_problem*>(ctx->enum_shells.back());
        ctx->enum_shells.pop_back();
        // (a list that grew for a degenerate problem is kept unless it is far larger than the default)
        const bool fits = knobs.list_pinned ? q->prefix.list_cap == knobs.list_cap
                                            : (q->prefix.list_cap >= knobs.list_cap && q->prefix.list_cap <= 64 * knobs.list_cap);
        if (fits) p = q; else enum_destroy(q);
    }
    const bool fresh = p == nullptr;
    if (fresh) {
        p = new lp_enum_problem();
        p->ctx = ctx;
    } else {   // forget what the previous problem left behind
        p->last_range = {};
        p->last_direct = {};
        p->dense_hint = false;
        p->exact_div = false;
        p->shard_rank = p->shard_world = -1;
    }
    p->knobs = knobs;
    p->complete = false;
    EnumDev& d = p->dev;
    d.m = m;
    d.n = n;
    d.lda = n + 1;
    d.rs = m > 16 ? ((m + 1) & ~1) : 16;   // row stride of the shared-prefix records (enum_tree.hpp: rec_rs)
    d.pad0 = 0;
    d.maximize = maximize ? 1 : 0;
    p->chunk_cap = 1 << 17;
    std::vector<double> Arow((size_t)m * d.lda, 0.0);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) Arow[(size_t)i * d.lda + j] = A[(size_t)j * m + i];
    std::vector<unsigned long long> binom((size_t)(kEnumMaxN + 1) * kBinomK, 0ULL);
    for (int i = 0; i <= kEnumMaxN; ++i)
        for (int k = 0; k < kBinomK; ++k) binom[(size_t)i * kBinomK + k] = lp_host_binom(i, k);
    // (a failed call below frees p with what it holds so far: p->complete is still false)
    std::unique_ptr<lp_enum_problem, void (*)(lp_enum_problem*)> owner(p, lp_enum_free);
    hipStream_t s = ctx->stream;
    if (fresh) {   // sized for the largest shape (m <= 32, n <= 64): a shell serves any later problem
        LP_HIP(ctx, hipMalloc(&p->dA, sizeof(double) * (size_t)kEnumMaxM * (kEnumMaxN + 1)));
        LP_HIP(ctx, hipMalloc(&p->db, sizeof(double) * (size_t)kEnumMaxM));
        LP_HIP(ctx, hipMalloc(&p->dc, sizeof(double) * (size_t)kEnumMaxN));
        LP_HIP(ctx, hipMalloc(&p->dbinom, sizeof(unsigned long long) * binom.size()));
        LP_HIP(ctx, hipMalloc(&p->d_pass, sizeof(EnumPassBlock)));
        d.result = &p->d_pass->result;
        LP_HIP(ctx, hipMalloc(&d.chunk_best, sizeof(double) * (size_t)(p->chunk_cap + 64)));
        LP_HIP(ctx, hipMalloc(&p->dvx, sizeof(double) * (kEnumMaxM + 1)));
        LP_HIP(ctx, hipMalloc(&p->dvi, sizeof(int) * (kEnumMaxM + 1)));
        LP_HIP(ctx, hipHostMalloc(&p->h_pass, sizeof(EnumPassBlock)));
        std::memset(p->h_pass, 0, sizeof(EnumPassBlock));
        p->h_result = &p->h_pass->result;
        p->h_list_count = &p->h_pass->list_count;
        p->h_overflow = &p->h_pass->overflow;
        p->h_level_counts = p->h_pass->level_counts;
        LP_HIP(ctx, hipEventCreate(&p->ev0));
        LP_HIP(ctx, hipEventCreate(&p->ev1));
        LP_HIP(ctx, hipMemcpyAsync(p->dbinom, binom.data(), sizeof(unsigned long long) * binom.size(),
                                   hipMemcpyHostToDevice, s));
    }
    LP_HIP(ctx, hipMemcpyAsync(p->dA, Arow.data(), sizeof(double) * Arow.size(), hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(p->db, b, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, s));
    LP_HIP(ctx, hipMemcpyAsync(p->dc, c, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    if (fresh) {   // shared-prefix path: small control words, the feasible list
        PrefixDev& pd = p->prefix;
        pd.level_counts = p->d_pass->level_counts;
        LP_HIP(ctx, hipMalloc(&pd.item_count, 2 * sizeof(int)));
        pd.overflow = &p->d_pass->overflow;
        LP_HIP(ctx, hipMalloc(&pd.root_cursor, 2 * sizeof(int)));
        LP_HIP(ctx, enum_list_alloc(p, knobs.list_cap));
        pd.list_count = &p->d_pass->list_count;
        if (!ctx->dcomb6 || !ctx->dcomb5 || !ctx->dcomb4) {   // (shape-independent: once per context)
            // the leaf kernels' 6-, 5- and 4-subsets of up to 22, 21 and 20 columns (first, second, third level)
            unsigned** dtab[3] = {&ctx->dcomb6, &ctx->dcomb5, &ctx->dcomb4};
            std::vector<unsigned> tab[3];
            for (int i = 0; i < 3; ++i) {
                tab[i] = subset_table(6 - i, 22 - i);
                LP_HIP(ctx, hipMalloc(dtab[i], sizeof(unsigned) * tab[i].size()));
                LP_HIP(ctx, hipMemcpyAsync(*dtab[i], tab[i].data(), sizeof(unsigned) * tab[i].size(), hipMemcpyHostToDevice, s));
            }
            LP_HIP(ctx, hipStreamSynchronize(s));  // the tables are locals
        }
        pd.comb6 = ctx->dcomb6;
        pd.comb5 = ctx->dcomb5;
        pd.comb4 = ctx->dcomb4;
    }
    LP_HIP(ctx, hipStreamSynchronize(s));
    d.A = p->dA;
    d.b = p->db;
    d.c = p->dc;
    d.binom = p->dbinom;
    p->complete = true;
    *problem_out = owner.release();
    return LP_OPTIMAL;
}

int lp_enum_range(lp_enum_problem* p, uint64_t rank_begin, uint64_t rank_end, int algo,
                  double* zbest_out, uint64_t* counts_out, lp_enum_stats* stats_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = check_range(p, rank_begin, rank_end);
    if (rc) return rc;
    p->last_range = {};
    if (algo != LP_ENUM_ALGO_AUTO && algo != LP_ENUM_ALGO_DIRECT && algo != LP_ENUM_ALGO_PREFIX)
        LP_FAIL(ctx, LP_BAD_ARG, "unknown enumeration algorithm id");
    if (rank_begin == rank_end) {   // an empty shard (more processes than subsets): nothing to launch
        if (zbest_out) *zbest_out = p->dev.maximize ? -INFINITY : INFINITY;
        if (counts_out)
            for (int k = 0; k < 3; ++k) counts_out[k] = 0;
        if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
        return LP_INFEASIBLE;
    }
    if (algo == LP_ENUM_ALGO_AUTO) {
        // the shared-prefix path pays for its breadth-first levels (0.13-0.25 ms of launches) from ~2^15
        // subsets on; with 32-row records (m > 16) from the start — the direct kernel's 32-lane form is
        // five times slower per subset than its 16-lane form (scripts/enum_threshold.py)
        const int shape = prefix_shape(p);
        const uint64_t least = shape == 3 ? (1ULL << 8) : (1ULL << 15);
        algo = (shape != 0 && rank_end - rank_begin >= least) ? LP_ENUM_ALGO_PREFIX : LP_ENUM_ALGO_DIRECT;
    }
    double score = -INFINITY;
    uint64_t counts[3] = {0, 0, 0};
    EnumRangeRecord rec;   // what this pass leaves for pass 2
    rec.begin = rank_begin;
    rec.end = rank_end;
    if (algo == LP_ENUM_ALGO_PREFIX) {
        if (!prefix_shape(p))
            LP_FAIL(ctx, LP_BAD_ARG, "shared-prefix enumeration needs 6 <= m <= 32 and n-m >= 2 (m >= 7 beyond 16 x 16; n-m <= 32 for m > 16)");
        rc = enum_prefix_pass(p, rank_begin, rank_end, &score, counts, stats_out, &rec.list);
        rec.kind = EnumRangeRecord::kList;
        uint64_t parts = 0;
        if (rc == kEnumRangeTooWide) {
            // more depth m-7 nodes than the level buffers hold: sub-ranges, a quarter over the
            // exact ratio (equal rank counts do not hold equal node counts)
            parts = p->split_hint + p->split_hint / 4 + 1;
        } else if (rc == kEnumListOverflow && *p->h_list_count * 2 <= rank_end - rank_begin) {
            // no memory for a list that long (or LP_ENUM_LIST_CAP pins its size).  Without the list
            // every feasible subset would be solved again from scratch for its objective, so once
            // more than half of the range is feasible the shared prefixes save nothing: that range
            // goes to the direct kernel as a whole; otherwise it is enumerated in sub-ranges, one
            // list at a time.
            parts = *p->h_list_count / (p->prefix.list_cap / 2) + 1;
        }
        if (parts) {
            rc = enum_prefix_chunked(p, rank_begin, rank_end, parts, &score, counts, stats_out, &rec.parts);
            rec.kind = EnumRangeRecord::kSubRanges;
        }
    }
    if (algo == LP_ENUM_ALGO_DIRECT || go_direct(rc)) {
        rc = lp_enum_direct_range(p, rank_begin, rank_end, &score, counts, stats_out);
        rec.kind = EnumRangeRecord::kNone;
    }
    if (rc) return rc;
    p->last_range = std::move(rec);
    if (zbest_out) *zbest_out = p->dev.maximize ? score : -score;
    if (counts_out)
        for (int k = 0; k < 3; ++k) counts_out[k] = counts[k];
    return counts[0] ? LP_OPTIMAL : LP_INFEASIBLE;
}

int lp_enum_first_within(lp_enum_problem* p, uint64_t rank_begin, uint64_t rank_end, double zstar,
                         double tol, uint64_t* rank_out) {
    if (!p || !rank_out) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = check_range(p, rank_begin, rank_end);
    if (rc) return rc;
    const double star = p->dev.maximize ? zstar : -zstar;
    const EnumRangeRecord& rec = p->last_range;
    const bool same_range = rec.begin == rank_begin && rec.end == rank_end;
    if (same_range && rec.kind == EnumRangeRecord::kList) {   // every feasible subset is listed
        if (star == rec.list.star && tol == rec.list.tol) {
            *rank_out = rec.list.first;   // already applied on the device by the range pass
            return LP_OPTIMAL;
        }
        return lp_enum_list_first(p, rec.list, star, tol, rank_out);
    }
    if (same_range && rec.kind == EnumRangeRecord::kSubRanges) {
        // the first sub-range that holds a qualifying subset is re-run to rebuild its list; the others
        // are skipped on their best score
        *rank_out = UINT64_MAX;
        for (const EnumSubRange& part : rec.parts) {
            if (!(part.best >= star - tol)) continue;
            uint64_t first = UINT64_MAX;
            if (part.direct) {
                rc = lp_enum_direct_first(p, part.begin, part.end, star, tol, &first);
            } else {
                double sc;
                uint64_t cn[3];
                EnumList list;
                rc = enum_prefix_pass(p, part.begin, part.end, &sc, cn, nullptr, &list);
                if (rc == LP_OPTIMAL) rc = lp_enum_list_first(p, list, star, tol, &first);
                else if (go_direct(rc)) rc = lp_enum_direct_first(p, part.begin, part.end, star, tol, &first);
            }
            if (rc) return rc;
            if (first != UINT64_MAX) {
                *rank_out = first;
                break;
            }
        }
        return LP_OPTIMAL;
    }
    return lp_enum_direct_first(p, rank_begin, rank_end, star, tol, rank_out);
}

int lp_enum_vertex(lp_enum_problem* p, uint64_t rank, int n_orig, double* x_out, int* basis_out,
                   double* obj_out, int* verdict_out) {
    if (!p) return LP_BAD_ARG;
    lp_context* ctx = p->ctx;
    LP_HIP(ctx, hipSetDevice(ctx->device));
    const EnumDev& d = p->dev;
    if (rank >= lp_host_binom(d.n, d.m)) LP_FAIL(ctx, LP_BAD_ARG, "rank >= C(n,m)");
    if (n_orig <= 0 || n_orig > d.n) LP_FAIL(ctx, LP_BAD_ARG, "bad original variable count");
    double xB[kEnumMaxM], z;
    int S[kEnumMaxM], verdict;
    int rc = lp_enum_direct_vertex(p, rank, xB, S, &z, &verdict);
    if (rc) return rc;
    if (x_out) {
        for (int j = 0; j < n_orig; ++j) x_out[j] = 0.0;
        for (int t = 0; t < d.m; ++t)
            if (S[t] < n_orig) x_out[S[t]] = xB[t];
    }
    if (basis_out)
        for (int t = 0; t < d.m; ++t) basis_out[t] = S[t];
    if (obj_out) *obj_out = z;
    if (verdict_out) *verdict_out = verdict;
    return LP_OPTIMAL;
}

int lp_enum_solve(lp_context* ctx, const double* A, int m, int n, const double* b,
                  const double* c, int maximize, int n_orig, double* x_out, int* basis_out,
                  uint64_t* rank_out, double* obj_out, uint64_t* counts_out) {
    if (!ctx) return LP_BAD_ARG;
    if (n_orig <= 0 || n_orig > n) LP_FAIL(ctx, LP_BAD_ARG, "bad original variable count");
    lp_enum_problem* p = nullptr;
    int rc = lp_enum_upload(ctx, A, m, n, b, c, maximize, &p);
    if (rc) return rc;
    // one participant, no exchange.  The vertex is always evaluated (obj_out is its objective, not pass 1's
    // optimum), which the sharded solve skips when neither x_out nor basis_out is asked for.
    std::vector<double> x;
    if (!x_out && !basis_out) {
        x.resize((size_t)n_orig);
        x_out = x.data();
    }
    rc = lp_enum_solve_sharded(nullptr, p, n_orig, x_out, basis_out, rank_out, obj_out, counts_out);
    lp_enum_free(p);
    return rc;
}

}  // extern "C"
