"""GPU parity for the shared in-LDS pivots and the item widths of the leaf kernels (k_enum_leaves<1> and <3> in
enum_leaf.hip): the shared-prefix path against the direct kernel and the oracle — optimum, tie-rule rank and counts,
bit for bit.  m = 7, 8, 9 with n - m = 10 .. 16: children with 9 .. 22 selectable columns, so the child pivot, the
group pivot and the sub-group pivot all occur, with tableaus of every width their copy loops end at.  A table-1 item
is 1024 subsets wide on ranges this small; LP_ENUM_CHUNK (read when a problem is uploaded) sets the widths a whole
range takes.
Every case has at least one feasible subset (checked with the oracle when the seeds were chosen, and asserted)."""
import contextlib
import functools

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import lpcases

pytestmark = pytest.mark.gpu

WINDOW = 300000   # subsets of a case at most: larger rank spaces are cut to their first WINDOW ranks, where the
                  # widest children are

SHAPES = [(m, m + d, 900 + 10 * m + d) for m in (7, 8, 9) for d in range(10, 17)]


@functools.lru_cache(maxsize=None)
def _reference(m, n, seed, kind):
    """(A, b, c, hi, oracle's (status, optimum, counts) and tie-rule rank over [0, hi)); read-only"""
    if kind == "random":
        A, b, c, _ = lpcases.random_lp(seed, m, n)
    else:
        rng = np.random.default_rng(seed)
        A = rng.integers(-2, 3, (m, n)).astype(float)
        A[rng.random((m, n)) < 0.35] = 0.0
        b = rng.integers(0, 4, m).astype(float)
        c = rng.integers(-2, 4, n).astype(float)
    hi = min(o.binom(n, m), WINDOW)
    ref = o.enum_range(A, b, c, True, 0, hi)
    assert ref[0] == o.OPTIMAL and ref[2][0] > 0
    k = o.enum_first_within(A, b, c, True, 0, hi, ref[1])
    for a in (A, b, c):
        a.setflags(write=False)
    return A, b, c, hi, ref, k


@contextlib.contextmanager
def _problem(ctx, A, b, c):
    """an uploaded problem, freed also when an assertion fails (the context must outlive its problems)"""
    p = ctx.enum_problem(A, b, c, True)
    try:
        yield p
    finally:
        p.free()


def _both(p, lo, hi):
    """(status, optimum, counts, tie-rule rank) of [lo, hi) on the shared-prefix path; the direct kernel must agree"""
    out = []
    for algo in (capi.ENUM_PREFIX, capi.ENUM_DIRECT):
        rc, z, counts, _ = p.range(lo, hi, algo)
        out.append((rc, z, counts, p.first_within(lo, hi, z) if rc == o.OPTIMAL else None))
    assert out[0] == out[1], (lo, hi, out)
    return out[0]


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_shared_pivots_match_direct_and_oracle(ctx, m, n, seed):
    A, b, c, hi, ref, k = _reference(m, n, seed, "random")
    with _problem(ctx, A, b, c) as p:
        assert _both(p, 0, hi) == (ref[0], ref[1], ref[2], k)


@pytest.mark.parametrize("chunk", [2048, 4096])
@pytest.mark.parametrize("m,n,seed", [(7, 23, 986), (8, 22, 994), (9, 21, 1002)])
def test_wide_items_match_direct_and_oracle(ctx, m, n, seed, chunk, monkeypatch):
    """The item widths of a whole range, on groups of up to C(21,5) = 20,349 subsets."""
    A, b, c, hi, ref, k = _reference(m, n, seed, "random")
    monkeypatch.setenv("LP_ENUM_CHUNK", str(chunk))
    with _problem(ctx, A, b, c) as p:
        assert _both(p, 0, hi) == (ref[0], ref[1], ref[2], k)


INTEGER_SHAPES = [(7, 17, 45), (7, 20, 44), (8, 19, 42), (9, 20, 42)]


@pytest.mark.parametrize("m,n,seed", INTEGER_SHAPES)
def test_exact_ties_and_zeros(ctx, m, n, seed):
    """Entries in {-2 .. 2}, a third of them zero: the magnitudes of a column tie at every step (the first row of the
    largest wins) and many prefixes are singular by an exactly-zero pivot (whole groups and sub-groups counted at the
    shared pivot).
    An exactly singular prefix must not send the pass to the plain divisions."""
    A, b, c, hi, ref, k = _reference(m, n, seed, "integer")
    assert ref[2][2] > 1000
    with _problem(ctx, A, b, c) as p:
        assert _both(p, 0, hi) == (ref[0], ref[1], ref[2], k)
        assert not p.exact_division


@pytest.mark.parametrize("m,n,seed", [(7, 18, 44), (8, 19, 42)])
def test_nan_and_inf_in_the_last_columns_and_the_rhs(ctx, m, n, seed):
    """A NaN is never a pivot maximum (a column of nothing else leaves the search at its default row: singular), and
    a solution that holds one is infeasible: the oracle's verdicts, subset by subset, also with wide items."""
    A, b, c, _, _, _ = _reference(m, n, seed, "integer")
    A, b = A.copy(), b.copy()
    A[2, n - 4] = np.nan
    A[m - 2, n - 2] = np.inf
    A[0, n - 9] = -np.inf
    total = o.binom(n, m)
    for rhs in (None, np.nan, np.inf):
        if rhs is not None:
            b[m - 3] = rhs
        st, z, counts = o.enum_range(A, b, c, True, 0, total)
        with _problem(ctx, A, b, c) as p:
            for algo in (capi.ENUM_PREFIX, capi.ENUM_DIRECT):
                rc, gz, gcounts, _ = p.range(0, total, algo)
                assert gcounts == counts and rc == st, (rhs, algo)
                assert gz == z or (np.isnan(gz) and np.isnan(z)), (rhs, algo)


def _group_start(n, m, a, j2):
    """m = 7 (the record is the root): rank of the first subset that begins with columns a, a + 1 + j2"""
    rank = sum(o.binom(n - 1 - q, m - 1) for q in range(a))
    return rank + sum(o.binom(n - 2 - a - q, m - 2) for q in range(j2))


@pytest.mark.parametrize("chunk", [1024, 2048, 4096])
def test_item_seams(ctx, chunk, monkeypatch):
    """m = 7, n = 23: 245,157 subsets, groups of C(15,5) = 3003 and more.  Rank windows that begin and end inside a
    group — on a multiple of 1024, 2048 and 4096 subsets from its start, one subset either side of it — and windows
    across two groups: the pieces of the rank space cut at those ranks add up to the whole (counts; the optimum is
    the largest piece's), and every piece is the oracle's."""
    m, n, seed = 7, 23, 986
    A, b, c, hi, ref, k = _reference(m, n, seed, "random")
    assert hi == o.binom(n, m)
    monkeypatch.setenv("LP_ENUM_CHUNK", str(chunk))
    cuts = {0, hi}
    for a, j2 in ((0, 0), (0, 1), (1, 0), (2, 3)):
        g = _group_start(n, m, a, j2)
        size = o.binom(n - 2 - a - j2, m - 2)
        assert size >= 3003
        for w in (1024, 2048, 4096):
            if w + 1 < size:
                cuts.update((g + w - 1, g + w, g + w + 1))
        cuts.update((g + size - 1, g + size + 1))   # a piece across the seam of two groups
    cuts = sorted(cuts)
    with _problem(ctx, A, b, c) as p:
        _seams(p, A, b, c, cuts, ref, k, _group_start(n, m, 0, 1))


def _seams(p, A, b, c, cuts, ref, k, g):
    zs, cs, firsts = [], np.zeros(3, dtype=np.int64), []
    for lo, up in zip(cuts[:-1], cuts[1:]):
        got = p.range(lo, up, capi.ENUM_PREFIX)[:3]
        assert got == o.enum_range(A, b, c, True, lo, up), (lo, up)
        zs.append(got[1])
        cs += got[2]
        if got[0] == o.OPTIMAL and got[1] == ref[1]:
            firsts.append(p.first_within(lo, up, got[1]))
    assert max(zs) == ref[1] and cs.tolist() == ref[2] and min(firsts) == k
    # windows that begin and end inside one group, and one that covers parts of two
    for lo, up in [(g + 1024, g + 2048), (g + 1023, g + 4097), (g + 2049, g + 6000), (g - 3000, g + 2048)]:
        want = o.enum_range(A, b, c, True, lo, up)
        assert p.range(lo, up, capi.ENUM_PREFIX)[:3] == want, (lo, up)
        assert p.range(lo, up, capi.ENUM_DIRECT)[:3] == want, (lo, up)
