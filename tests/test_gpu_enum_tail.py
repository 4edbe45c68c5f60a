"""GPU parity for the deep end of the shared-prefix enumeration: the subsets inside the last columns of every depth
m-7 record (k_enum_thin in enum_leaf.hip) against the direct kernel and the oracle — optimum, tie-rule rank and
counts, bit for bit.  Shapes are the smallest that reach every branch: m = 7 (the record is the root, depth 0),
m = 8 and 9, and n - m = 7 .. 11, so that records with 7, 8, 9, 10 and more selectable columns occur in one problem.
Every case has at least one feasible subset (checked with the oracle when the seeds were chosen, and asserted)."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import lpcases

pytestmark = pytest.mark.gpu


SHAPES = [(m, m + d, 700 + 10 * m + d) for m in (7, 8, 9) for d in (7, 8, 9, 10, 11)]


@functools.lru_cache(maxsize=None)
def _case(m, n, seed):
    """(A, b, c, total, oracle's (status, optimum, counts) and tie-rule rank over the whole rank space); read-only"""
    A, b, c, _ = lpcases.random_lp(seed, m, n)
    total = o.binom(n, m)
    ref = o.enum_range(A, b, c, True, 0, total)
    assert ref[0] == o.OPTIMAL and ref[2][0] > 0
    k = o.enum_first_within(A, b, c, True, 0, total, ref[1])
    for a in (A, b, c):
        a.setflags(write=False)
    return A, b, c, total, ref, k


def _both(p, lo, hi):
    """(status, optimum, counts, tie-rule rank) of [lo, hi) on the shared-prefix path; the direct kernel must agree"""
    out = []
    for algo in (capi.ENUM_PREFIX, capi.ENUM_DIRECT):
        rc, z, counts, _ = p.range(lo, hi, algo)
        out.append((rc, z, counts, p.first_within(lo, hi, z) if rc == o.OPTIMAL else None))
    assert out[0] == out[1], (lo, hi, out)
    return out[0]


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_tail_matches_direct_and_oracle(ctx, m, n, seed):
    A, b, c, total, ref, k = _case(m, n, seed)
    p = ctx.enum_problem(A, b, c, True)
    assert _both(p, 0, total) == (ref[0], ref[1], ref[2], k)
    p.free()


def test_tail_end_of_the_c32_16_rank_space(ctx):
    """The last 4,000 ranks of C(32,16): only deep records with few selectable columns meet the window."""
    m, n, seed = 16, 32, 0
    A, b, c, _ = lpcases.random_lp(seed, m, n)
    total = o.binom(n, m)
    lo, hi = total - 4000, total
    ref = o.enum_range(A, b, c, True, lo, hi)
    assert ref[0] == o.OPTIMAL and ref[2][0] > 0
    p = ctx.enum_problem(A, b, c, True)
    assert _both(p, lo, hi) == (ref[0], ref[1], ref[2], o.enum_first_within(A, b, c, True, lo, hi, ref[1]))
    p.free()


def _record_end(n, m, a):
    """rank behind the last subset whose first column is a (m = 8: the depth m-7 record with prefix {a})"""
    return sum(o.binom(n - 1 - q, m - 1) for q in range(a + 1))


def test_windows_inside_one_records_tail(ctx):
    """begin and end inside the last subsets of one record: the range test is per subset.  The windows lie inside
    the last 8, the last 36 and the last 120 ranks of a record, end on its last rank, and cross into the next."""
    m, n, seed = 8, 19, 791
    A, b, c, total, _, _ = _case(m, n, seed)
    p = ctx.enum_problem(A, b, c, True)
    for a in (0, 2, 5):   # records with 18, 16 and 13 selectable columns
        e = _record_end(n, m, a)
        for lo, hi in [(e - 6, e - 2), (e - 8, e), (e - 30, e - 9), (e - 36, e - 35), (e - 110, e - 40), (e - 121, e - 119),
                       (e - 1, e), (e - 3, e + 2), (e - 130, e + 130)]:
            want = o.enum_range(A, b, c, True, lo, hi)
            got = p.range(lo, hi, capi.ENUM_PREFIX)[:3]
            assert got == want, (a, lo - e, hi - e)
            assert p.range(lo, hi, capi.ENUM_DIRECT)[:3] == want, (a, lo - e, hi - e)
            if want[0] == o.OPTIMAL:
                assert p.first_within(lo, hi, want[1]) == o.enum_first_within(A, b, c, True, lo, hi, want[1])
    p.free()


@pytest.mark.parametrize("m,n,seed", [(7, 17, 780), (9, 20, 801)])
def test_tail_shards_compose(ctx, m, n, seed):
    A, b, c, total, ref, k = _case(m, n, seed)
    p = ctx.enum_problem(A, b, c, True)
    for parts in (2, 3, 8, 61):
        cuts = [total * q // parts for q in range(parts + 1)]
        zs, cs, firsts = [], np.zeros(3, dtype=np.int64), []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            rc, z, counts, _ = p.range(lo, hi, capi.ENUM_PREFIX)
            zs.append(z)
            cs += counts
            if rc == o.OPTIMAL and z == ref[1]:
                firsts.append(p.first_within(lo, hi, z))
        assert max(zs) == ref[1] and cs.tolist() == ref[2] and min(firsts) == k, parts
    p.free()


def test_tail_singular_nan_and_inf_in_the_last_columns(ctx):
    """Duplicate and zero columns among the last ten (whole tails singular), NaN and inf entries there (a NaN is never
    a pivot maximum; a solution that holds one is infeasible): the oracle's verdicts, subset by subset."""
    m, n, seed = 8, 18, 311
    A, b, c, _ = lpcases.random_lp(seed, m, n)
    A[:, n - 2] = A[:, n - 5]
    A[:, n - 7] = 0.0
    A[2, n - 4] = np.nan
    A[5, n - 3] = np.inf
    total = o.binom(n, m)
    st, z, counts = o.enum_range(A, b, c, True, 0, total)
    assert st == o.OPTIMAL and counts[0] > 0 and counts[2] > 1000
    p = ctx.enum_problem(A, b, c, True)
    assert _both(p, 0, total) == (st, z, counts, o.enum_first_within(A, b, c, True, 0, total, z))
    lo, hi = total - 3000, total - 2
    assert p.range(lo, hi, capi.ENUM_PREFIX)[:3] == o.enum_range(A, b, c, True, lo, hi)
    p.free()


def test_tail_lists_many_feasible_subsets(ctx, monkeypatch):
    """b = 0: every non-singular subset is feasible, the tail lanes list all of theirs and the list (300 entries to
    start with) grows."""
    monkeypatch.setenv("LP_ENUM_LIST_START", "300")
    m, n, seed = 8, 17, 779
    A, b, c, _ = lpcases.random_lp(seed, m, n)
    b = np.zeros_like(b)
    total = o.binom(n, m)
    ref = o.enum_range(A, b, c, True, 0, total)
    assert ref[0] == o.OPTIMAL and ref[2][0] > 300
    p = ctx.enum_problem(A, b, c, True)
    assert _both(p, 0, total) == (ref[0], ref[1], ref[2], o.enum_first_within(A, b, c, True, 0, total, ref[1]))
    lo, hi = total - 900, total
    ref2 = o.enum_range(A, b, c, True, lo, hi)
    assert ref2[2][0] > 300
    assert _both(p, lo, hi) == (ref2[0], ref2[1], ref2[2], o.enum_first_within(A, b, c, True, lo, hi, ref2[1]))
    p.free()


@pytest.mark.parametrize("m,n,seed", [(7, 16, 779), (8, 18, 790), (9, 19, 800)])
def test_tail_plain_division_agrees(ctx, m, n, seed, monkeypatch):
    A, b, c, total, ref, k = _case(m, n, seed)
    p = ctx.enum_problem(A, b, c, True)
    assert p.range(0, total, capi.ENUM_PREFIX)[:3] == ref and not p.exact_division
    p.free()
    monkeypatch.setenv("LP_ENUM_EXACT_DIV", "1")
    q = ctx.enum_problem(A, b, c, True)
    assert q.range(0, total, capi.ENUM_PREFIX)[:3] == ref and q.exact_division
    assert q.first_within(0, total, ref[1]) == k
    q.free()


@pytest.mark.parametrize("m,n,seed", [(7, 15, 778), (8, 17, 789)])
def test_tail_raises_the_range_flag(ctx, m, n, seed):
    """Scaled by 2^-510 every pivot lies outside the fast reciprocal's range; a window at the end of the rank space is
    the tail kernel's alone (its 8 subsets lie inside the last 8 columns of their records, where every child is too
    narrow for the item tables), so the flag is its own."""
    A, b, c, _, _, _ = _case(m, n, seed)
    A, b = A * 2.0 ** -510, b * 2.0 ** -510
    total = o.binom(n, m)
    lo = total - 8
    ref = o.enum_range(A, b, c, True, lo, total)
    assert ref[0] == o.OPTIMAL and ref[2][0] > 0
    p = ctx.enum_problem(A, b, c, True)
    assert not p.exact_division
    assert p.range(lo, total, capi.ENUM_PREFIX)[:3] == ref
    assert p.exact_division
    assert p.range(lo, total, capi.ENUM_DIRECT)[:3] == ref
    whole = o.enum_range(A, b, c, True, 0, total)
    assert p.range(0, total, capi.ENUM_PREFIX)[:3] == whole
    p.free()


def test_tail_packing_loses_nothing_under_repetition(ctx):
    """One small range 30 times over: the dense packing of the tail lanes must lose no subset and double none."""
    m, n, seed = 9, 20, 801
    A, b, c, total, _, _ = _case(m, n, seed)
    lo, hi = total // 5 + 3, total - total // 9
    ref = o.enum_range(A, b, c, True, lo, hi)
    assert sum(ref[2]) == hi - lo and ref[2][0] > 0
    p = ctx.enum_problem(A, b, c, True)
    for _ in range(30):
        assert p.range(lo, hi, capi.ENUM_PREFIX)[:3] == ref
    p.free()
