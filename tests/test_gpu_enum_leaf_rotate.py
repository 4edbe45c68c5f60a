"""GPU parity for the row rotation of the leaf kernels' per-subset routine (enum_leaf.hip: leaf_verdict_impl, whose
rotating steps move the chosen row as 64-bit moves under the lane mask): the shapes that reach the seven-, six-, five-
and four-column routines, the knobs that send a subset to another kernel with the same routine, the general kernel,
the plain-division instantiations, and exact ties of the largest entry in the rotating steps.  Every comparison is bit
for bit — status, optimum, tie-rule rank, the three counts (whose sum is the window) and the winning vertex — between
the shared-prefix path and the direct kernel, and on the small shapes the CPU oracle.

A rotation can go wrong only per pivot position, so a numpy replay of the routine's pivot order (_replay) shows on the
CPU that the inputs below put the chosen row at every position p of every rotating step of every routine, and that
the 2x2 block takes its second row as well as its first.  The seeds were picked with that replay.

Where the rotations live.  Every leaf kernel, the general one (k_enum_generic_leaves) included, reads its rows
permuted (PERM): steps 0 and 1 choose their rows before loading, and the routine rotates from step 2 on — KD-t+1 = 4,
5 or 6 values a row.  The UNPERMUTED routine, which rotates at every step from 0 on (8 and 7 values a row at steps 0
and 1), has one caller: the list evaluation k_enum_eval_records, seven columns a lane, which scores the FEASIBLE
subsets from their depth m-7 records.  So the census of steps 0 and 1 runs over feasible subsets only
(test_census_of_list_evaluation), and since a pass reports only the best objective, every subset of that census is
scored alone through a one-subset window and compared with the oracle's objective for it
(test_list_evaluation_scores_each_subset)."""
import functools
import itertools

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import lpcases

gpu = pytest.mark.gpu   # on the tests that run a kernel; the censuses run on the CPU, in the suite without a GPU too

# Copies of enum_leaf.hip's constants of the same names (THIN_TAIL, kGrandMin = LP_GRAND_MIN, kGreatMin = LP_GREAT_MIN);
# _routine below restates the dispatch of that file's header comment.  test_constants_match_the_source reads them back
# from the source, so that a change there fails here instead of leaving the census on stale labels.
THIN_TAIL = 9    # a child with fewer selectable columns is finished from its record, 7 columns a lane
GRAND_MIN = 10   # a group with at least 10 selectable columns gets a second pivot, 5 columns a lane
GREAT_MIN = 9    # a sub-group with at least 9 gets a third, 4 columns a lane


def test_constants_match_the_source():
    import os
    import re
    src = open(os.path.join(os.path.dirname(capi.__file__), "csrc", "enum_leaf.hip")).read()
    assert int(re.search(r"constexpr int THIN_TAIL = (\d+);", src).group(1)) == THIN_TAIL
    assert int(re.search(r"#define LP_GRAND_MIN (\d+)", src).group(1)) == GRAND_MIN
    assert int(re.search(r"#define LP_GREAT_MIN (\d+)", src).group(1)) == GREAT_MIN


def _problem(ctx, monkeypatch, A, b, c, **env):
    """a problem whose knobs (read at upload) are env"""
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, str(v))
        return ctx.enum_problem(A, b, c, True)


def _result(p, lo, hi, algo):
    """(status, optimum, counts, tie-rule rank, winning vertex and basis as bytes) of [lo, hi)"""
    rc, z, counts, _ = p.range(lo, hi, algo)
    if rc != o.OPTIMAL:
        return rc, z, counts, None, None
    k = p.first_within(lo, hi, z)
    v = p.vertex(k)
    return rc, z, counts, k, (v["x"].tobytes(), v["basis"].tobytes(), v["obj"])


@functools.lru_cache(maxsize=None)
def _oracle(key, lo, hi):
    A, b, c = _inputs(key)
    st, z, counts = o.enum_range(A, b, c, True, lo, hi)
    return st, z, counts, (o.enum_first_within(A, b, c, True, lo, hi, z) if st == o.OPTIMAL else None)


def _both_ways(ctx, monkeypatch, key, windows, oracle=False, **env):
    """every window on the shared-prefix path, on the direct kernel and (oracle=True) on the CPU oracle"""
    A, b, c = _inputs(key)
    p = _problem(ctx, monkeypatch, A, b, c, **env)
    got = [_result(p, lo, hi, capi.ENUM_PREFIX) for lo, hi in windows]
    direct = [_result(p, lo, hi, capi.ENUM_DIRECT) for lo, hi in windows]
    p.free()
    for w, g, d in zip(windows, got, direct):
        assert sum(g[2]) == w[1] - w[0], w
        assert g == d, (w, g[:4], d[:4])
        if oracle:
            assert g[:4] == _oracle(key, *w), w
    return got


TIE_SHAPE = (8, 20, 1701)
TIE_ROWS = (2, 5)   # the tie input: row 5 is the negation of row 2 outside the last two columns


@functools.lru_cache(maxsize=None)
def _inputs(key):
    """key = (kind, m, n, seed).  "lp": lpcases.random_lp = [dense | I] with the columns reversed, so that the last
    ones — the columns the leaf kernels' lanes choose from — are the dense ones.  "dense": uniform entries in (-1, 1) and
    b = A x0 with x0 > 0 (feasible subsets whose pivot rows fall anywhere).  "tie": the same, row
    TIE_ROWS[1] the exact negation of row TIE_ROWS[0] outside the last two columns: until one of the two is a pivot row
    (or one of the last two columns a pivot column) their entries stay exact negations of each other through every
    elimination — rounding is symmetric in the sign — so wherever they hold the largest entry of a pivot column, they
    tie exactly and the first of them, row TIE_ROWS[0], must be chosen."""
    kind, m, n, seed = key
    if kind == "lp":
        A, b, c, _ = lpcases.random_lp(seed, m, n)
        A, c = np.ascontiguousarray(A[:, ::-1]), np.ascontiguousarray(c[::-1])
    else:   # "tie", and "dense": the same without the tie
        rng = np.random.default_rng(seed)
        A = rng.uniform(-1.0, 1.0, (m, n))
        i, j = TIE_ROWS
        if kind == "tie":
            A[j, :n - 2] = -A[i, :n - 2]
        b = A @ rng.uniform(0.5, 1.5, n)
        c = rng.uniform(-1.0, 1.0, n)
    for a in (A, b, c):
        a.setflags(write=False)
    return A, b, c


def _subsets(n, m, lo, hi):
    """the subsets of ranks [lo, hi), ascending columns, lexicographic order"""
    if hi - lo > 50000:
        allc = np.array(list(itertools.combinations(range(n), m)), dtype=np.int64)
        return allc[lo:hi]
    out = np.empty((hi - lo, m), dtype=np.int64)
    s = list(o.unrank(n, m, lo))
    for k in range(hi - lo):
        out[k] = s
        i = m - 1
        while i >= 0 and s[i] == n - m + i:
            i -= 1
        if i < 0:
            break
        s[i] += 1
        for q in range(i + 1, m):
            s[q] = s[q - 1] + 1
    return out


def _replay(A, subsets):
    """The pivot order of the per-subset elimination (oracle/lp_oracle.c: orc_enum_subset, which the routine follows):
    Gauss-Jordan over the subset's columns in ascending order, the first row of largest |entry| among the rows not yet
    used.  Returns pos[k, s], the position of step s's row among the unused rows in ascending order (what the routine
    rotates by), tie[k, s], whether the largest |entry| was held by more than one row, and second[k], whether the 2x2
    block takes the second of its two rows.  (numpy rounds a multiply-add twice where the kernels fuse it: near-ties
    may fall differently, which does not matter to a census of positions.)"""
    m = A.shape[0]
    K = len(subsets)
    W = np.ascontiguousarray(A[:, subsets].transpose(1, 0, 2))   # (K, m, m)
    used = np.zeros((K, m), dtype=bool)
    pos = np.zeros((K, m - 2), dtype=np.int64)
    tie = np.zeros((K, m - 2), dtype=bool)
    ar = np.arange(K)
    rows = np.arange(m)[None, :]
    with np.errstate(all="ignore"):
        for s in range(m - 2):
            col = np.abs(W[:, :, s])
            col[used] = -1.0
            col[np.isnan(col)] = -1.0
            p = np.argmax(col, axis=1)                           # the first of the largest
            big = col[ar, p]
            tie[:, s] = ((col == big[:, None]).sum(axis=1) > 1) & (big > 0.0)
            pos[:, s] = (~used & (rows < p[:, None])).sum(axis=1)
            prow = W[ar, p, :].copy()
            inv = 1.0 / prow[:, s]
            l = -(W[:, :, s] * inv[:, None])
            l[ar, p] = 0.0
            W = W + l[:, :, None] * prow[:, None, :]
            W[ar, p, :] = prow * inv[:, None]
            used[ar, p] = True
        last = np.argsort(used, axis=1, kind="stable")[:, :2]    # the two unused rows, ascending
        second = np.abs(W[ar, last[:, 1], m - 2]) > np.abs(W[ar, last[:, 0], m - 2])
    return pos, tie, second


def _routine(n, m, subsets, tuned=True):
    """columns per lane of the routine that finishes each subset (enum_leaf.hip's header): by the record's child column
    a, the first remaining column a2 and the next a3; the general kernel (more than 16 rows) takes 7 throughout"""
    if not tuned:
        return np.full(len(subsets), 7)
    a, a2, a3 = subsets[:, m - 7], subsets[:, m - 6], subsets[:, m - 5]
    return np.where(a >= n - THIN_TAIL, 7,
                    np.where(n - 1 - a2 >= GRAND_MIN, np.where(n - 1 - a3 >= GREAT_MIN, 4, 5), 6))


def _census(A, n, m, windows, tuned=True, ties=False):
    """asserts that the subsets of the windows put the chosen row at every position of every rotating step (t >= 2) of
    every routine they reach, take both rows in the 2x2 block, and (ties=True) tie exactly for the largest entry at
    every rotating step; returns the routines reached"""
    subsets = np.concatenate([_subsets(n, m, lo, hi) for lo, hi in windows])
    pos, tie, second = _replay(A, subsets)
    kd = _routine(n, m, subsets, tuned)
    reached = sorted(set(kd.tolist()))
    for K in reached:
        sel = kd == K
        assert second[sel].any() and not second[sel].all(), K
        for t in range(2, K - 2):
            s = m - K + t
            assert set(pos[sel, s].tolist()) == set(range(K - t)), (K, t, sorted(set(pos[sel, s].tolist())))
            if ties:
                assert tie[sel, s].any(), (K, t)
    return reached


def _windows(n, m):
    """the whole range and a few windows: across the first record's children (six, five and four columns a lane), and
    the tail of the range, where every subset lies inside the last columns (seven)"""
    total = o.binom(n, m)
    return [(0, total), (total // 7, total // 7 + 20011), (total // 2 - 5000, total // 2 + 9001), (total - 3003, total)]


# (m, n, seed): picked on the CPU so that the census below holds on the partial windows alone
SHAPES = [(8, 20, 1701), (7, 18, 1707)]


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_census_of_pivot_positions(m, n, seed):
    """(no kernel runs: the coverage the other tests rely on — every routine, every position, both 2x2 rows, on the
    windows without the whole range, and exact ties at every rotating step of the tie input)"""
    key = ("lp", m, n, seed)
    assert _census(_inputs(key)[0], n, m, _windows(n, m)[1:]) == [4, 5, 6, 7]
    if (m, n) == TIE_SHAPE[:2]:
        A = _inputs(("tie",) + TIE_SHAPE)[0]
        assert _census(A, n, m, [(0, o.binom(n, m))], ties=True) == [4, 5, 6, 7]


@gpu
@pytest.mark.parametrize("env", [{}, {"LP_ENUM_PARENT_TAILS": 1}, {"LP_ENUM_LEAF_QUADS": 0}, {"LP_ENUM_EXACT_DIV": 1}],
                         ids=["default", "parent_tails", "no_quads", "exact_div"])
def test_small_shape_all_routines(ctx, monkeypatch, env):
    """m = 8, n = 20: whole range and windows, the oracle on all of them; the knobs move subsets between kernels that
    share the routine (k_enum_parent_tails, k_enum_leaves<1>) or select the plain-division instantiations"""
    m, n, seed = SHAPES[0]
    got = _both_ways(ctx, monkeypatch, ("lp", m, n, seed), _windows(n, m), oracle=True, **env)
    assert got[0][0] == o.OPTIMAL and got[0][2][0] > 0


@gpu
def test_root_record_shape(ctx, monkeypatch):
    """m = 7, n = 18: the root record alone"""
    m, n, seed = SHAPES[1]
    got = _both_ways(ctx, monkeypatch, ("lp", m, n, seed), _windows(n, m), oracle=True)
    assert got[0][0] == o.OPTIMAL and got[0][2][0] > 0


GENERAL = (18, 30, 1705)
GENERAL_WINDOW = (40_000_000, 40_200_000)


@gpu
def test_general_kernel_window(ctx, monkeypatch):
    """m = 18, n = 30 (beyond the tuned kernels' 16 rows): a window of 200 k subsets on the general leaf kernel, seven
    columns a lane; the census on its first 20,000"""
    m, n, seed = GENERAL
    key = ("lp", m, n, seed)
    lo, hi = GENERAL_WINDOW
    assert _census(_inputs(key)[0], n, m, [(lo, lo + 20000)], tuned=False) == [7]
    _both_ways(ctx, monkeypatch, key, [GENERAL_WINDOW, (lo + 777, lo + 50001)])


@gpu
def test_exact_ties_in_rotating_steps(ctx, monkeypatch):
    """one row the negation of another outside two columns: exact ties of the largest entry in the rotating steps of
    every routine (test_census_of_pivot_positions); the first-of-largest rule must give the oracle's row — a wrong row
    changes the vertex or the verdict of the subsets behind it"""
    m, n, _ = TIE_SHAPE
    total = o.binom(n, m)
    got = _both_ways(ctx, monkeypatch, ("tie",) + TIE_SHAPE, [(0, total), (total // 3, total // 3 + 30011)], oracle=True)
    assert got[0][0] == o.OPTIMAL and got[0][2][0] > 0 and got[0][2][2] > 0


# ---- the unpermuted routine: k_enum_eval_records on the feasible subsets

LIST_SHAPES = [(8, 20, 1711), (7, 18, 1711)]   # (m, n, seed) of "dense" inputs, picked with _list_census
PER_POSITION = 6                               # subsets scored alone per (step, position)


@functools.lru_cache(maxsize=None)
def _feasible(key, lo, hi):
    """(ranks, subsets, objectives) of the subsets of [lo, hi) that the oracle finds feasible: candidates by a batched
    numpy solve with a wide margin, each then decided by oracle/lp_oracle.c: orc_enum_subset — a subset the margin
    misses only makes the census smaller"""
    A, b, c = _inputs(key)
    m, n = A.shape
    subsets = _subsets(n, m, lo, hi)
    with np.errstate(all="ignore"):
        x = np.linalg.solve(A[:, subsets].transpose(1, 0, 2), np.broadcast_to(b[None, :, None], (len(subsets), m, 1)))[..., 0]
    cand = np.flatnonzero(np.isfinite(x).all(axis=1) & (x >= -1e-6).all(axis=1))
    keep, zs = [], []
    for k in cand:
        st, _, z = o.enum_subset(A, b, c, subsets[k])
        if st == o.SUBSET_FEASIBLE:
            keep.append(k)
            zs.append(z)
    keep = np.array(keep, dtype=np.int64)
    return lo + keep, subsets[keep], np.array(zs)


def _list_census(key, lo, hi, full=True):
    """the list evaluation's seven steps on the feasible subsets of [lo, hi): local step t = global step m-7+t, five
    of them rotating (t = 0..4: 7-t rows, 8-t values a row).  full: asserts every position 0..6-t at every t and both
    rows of the 2x2 block.  Returns {(t, position): indices into _feasible(key, lo, hi)}, at most PER_POSITION each"""
    A = _inputs(key)[0]
    m = A.shape[0]
    ranks, subsets, _ = _feasible(key, lo, hi)
    pos, _, second = _replay(A, subsets)
    picks = {}
    for t in range(5):
        reached = pos[:, m - 7 + t]
        if full:
            assert set(reached.tolist()) == set(range(7 - t)), (t, sorted(set(reached.tolist())))
        for p in sorted(set(reached.tolist())):
            picks[(t, p)] = np.flatnonzero(reached == p)[:PER_POSITION]
    if full:
        assert second.any() and not second.all()
    return picks


@pytest.mark.parametrize("m,n,seed", LIST_SHAPES)
def test_census_of_list_evaluation(m, n, seed):
    """(no kernel runs) the feasible subsets of the "dense" inputs put the chosen row at every position of steps 0 .. 4
    of the unpermuted seven-column routine — steps 0 and 1, eight and seven values a row, exist nowhere else"""
    picks = _list_census(("dense", m, n, seed), 0, o.binom(n, m))
    assert len(picks) == 7 + 6 + 5 + 4 + 3


def _scored_alone(ctx, monkeypatch, key, lo, hi, picks):
    """every picked subset as a window of its own on the shared-prefix path (one list entry, scored by
    k_enum_eval_records from its record): status, objective bit for bit the oracle's for that subset, rank, counts"""
    A, b, c = _inputs(key)
    ranks, _, zs = _feasible(key, lo, hi)
    p = _problem(ctx, monkeypatch, A, b, c)
    for (t, q), idx in sorted(picks.items()):
        for k in idx:
            r = int(ranks[k])
            rc, z, counts, _ = p.range(r, r + 1, capi.ENUM_PREFIX)
            assert (rc, counts) == (o.OPTIMAL, [1, 0, 0]) and z == zs[k], (t, q, r, rc, z, zs[k], counts)
            assert p.first_within(r, r + 1, z) == r
    p.free()


@gpu
@pytest.mark.parametrize("m,n,seed", LIST_SHAPES)
def test_list_evaluation_scores_each_subset(ctx, monkeypatch, m, n, seed):
    """the census' subsets, PER_POSITION per (step, position), each scored alone; then the whole range both ways"""
    key = ("dense", m, n, seed)
    total = o.binom(n, m)
    _scored_alone(ctx, monkeypatch, key, 0, total, _list_census(key, 0, total))
    got = _both_ways(ctx, monkeypatch, key, [(0, total)], oracle=True)
    assert got[0][2][0] == len(_feasible(key, 0, total)[0])


LIST_GENERAL = ("dense", 18, 30, 1716)


@gpu
def test_list_evaluation_general_shape(ctx, monkeypatch):
    """m = 18, n = 30: k_enum_eval_records<32> (32-row records, run-time column stride) on the 56 feasible subsets among
    the first 20,000 of the general window, each scored alone: they reach six of the seven positions at step 0 and
    every position at steps 1 .. 4 (picked on the CPU)"""
    lo = GENERAL_WINDOW[0]
    picks = _list_census(LIST_GENERAL, lo, lo + 20000, full=False)
    assert [sum(1 for (tt, _) in picks if tt == t) for t in range(5)] == [6, 6, 5, 4, 3], sorted(picks)
    _scored_alone(ctx, monkeypatch, LIST_GENERAL, lo, lo + 20000, picks)
    _both_ways(ctx, monkeypatch, LIST_GENERAL, [(lo, lo + 20000)])
