"""GPU parity for table 1 of the shared-prefix enumeration (enum_leaf.hip: k_enum_leaves<3>) on the shapes and windows
that separate its paths: groups (depth m-5 nodes) of 10 .. 20 selectable columns, whose sub-groups get a third in-LDS
pivot and four columns per lane and whose tails get five; windows that begin and end inside a sub-group, inside a
group's tail and inside an item packed of several groups; inputs on which phase 2 of the per-subset routine
(leaf_verdict, unrolled over the tableau's rows in the tuned kernels) runs for many rows in many lanes.  Every
comparison is bit for bit — status, optimum, tie-rule rank, the three counts (whose sum is the window) and the winning
vertex — between the shared-prefix path and the direct kernel, and on the two small shapes the CPU oracle."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import lpcases

pytestmark = pytest.mark.gpu

GREAT_MIN = 9    # ... kGreatMin: a sub-group (depth m-4 node) with at least 9 selectable columns gets the third pivot


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


def _oracle(A, b, c, lo, hi):
    st, z, counts = o.enum_range(A, b, c, True, lo, hi)
    return st, z, counts, (o.enum_first_within(A, b, c, True, lo, hi, z) if st == o.OPTIMAL else None)


def _both_ways(ctx, monkeypatch, A, b, c, windows, oracle=False, **env):
    """every window on the shared-prefix path, on the direct kernel and (oracle=True) on the CPU oracle"""
    p = _problem(ctx, monkeypatch, A, b, c, **env)
    got = [_result(p, lo, hi, capi.ENUM_PREFIX) for lo, hi in windows]
    direct = [_result(p, lo, hi, capi.ENUM_DIRECT) for lo, hi in windows]
    p.free()
    for w, g, d in zip(windows, got, direct):
        assert sum(g[2]) == w[1] - w[0], w
        assert g == d, (w, g[:4], d[:4])
        if oracle:
            assert g[:4] == _oracle(A, b, c, *w), w
    return got


@functools.lru_cache(maxsize=None)
def _lp(m, n, seed):
    """random_lp is [dense | I]: an odd seed reverses the columns, so that the last ones — the columns the leaf
    kernels' lanes choose from — are the dense ones (the vertices and their count are the same)"""
    A, b, c, _ = lpcases.random_lp(seed, m, n)
    if seed % 2:
        A, c = np.ascontiguousarray(A[:, ::-1]), np.ascontiguousarray(c[::-1])
    for a in (A, b, c):
        a.setflags(write=False)
    return A, b, c


def _node(n, m, prefix):
    """[first, end) of the ranks of the subsets below the node `prefix` (ascending columns)"""
    rank, lo = 0, 0
    for k, col in enumerate(prefix):
        rank += sum(o.binom(n - 1 - q, m - 1 - k) for q in range(lo, col))
        lo = col + 1
    return rank, rank + o.binom(n - lo, m - len(prefix))


def _group(n, m, a, a2):
    """the group (depth m-5 node) below the first record's child on column a with first remaining column a2: its
    selectable columns, [first, end), the first rank of its tail (the subsets no sub-group takes)"""
    g = tuple(range(m - 7)) + (a, a2)
    R2 = n - 1 - a2
    first, end = _node(n, m, g)
    a3_tail = n - GREAT_MIN            # the first a3 that leaves fewer than 9 selectable columns
    return R2, first, end, _node(n, m, g + (a3_tail,))[0]


def _sub(n, m, a, a2, a3):
    return _node(n, m, tuple(range(m - 7)) + (a, a2, a3))


def _windows(m, n):
    """windows that begin and end inside a sub-group, inside a group's tail and inside a packed item of several
    groups, in groups of 16, 11 and 10 selectable columns"""
    a = m - 7                            # first child of the first record
    total = o.binom(n, m)
    w = [(0, total)]
    a2 = n - 1 - 16                      # 16 selectable columns: sub-groups with 15 .. 9 columns, then the tail
    R2, first, end, tail = _group(n, m, a, a2)
    assert R2 == 16 and first < tail < end
    s0, e0 = _sub(n, m, a, a2, a2 + 1)   # its first sub-group: C(15, 4) = 1365 subsets
    assert s0 == first and e0 - s0 == 1365
    s3 = _sub(n, m, a, a2, a2 + 4)[0]
    w += [(s0 + 37, s0 + 1000), (s0 + 64, s0 + 128), (s0 + 5, s0 + 6), (e0 - 1, e0 + 1),   # inside a sub-group, a seam
          (s0 + 700, s3 + 77), (s3 + 77, tail + 3),                                        # across sub-groups, into the tail
          (tail + 3, tail + 100), (tail + 70, end - 1), (tail - 1, tail + 1), (first, end)]
    # the two smallest groups: 11 columns (sub-groups of 210 and 126 subsets) and 10 (one sub-group and a tail)
    for cols in (11, 10):
        R2, first, end, tail = _group(n, m, a, n - 1 - cols)
        assert R2 == cols and end - first == o.binom(cols, 5)
        w += [(first, end), (first + 10, end - 10), (first + 100, tail + 60), (tail + 1, end - 1)]
    # small groups share a packed item: from inside the 12-column group to inside the 10-column group, and from the
    # tail of one child's last group into the next child's groups
    f12, f10 = _group(n, m, a, n - 13)[1], _group(n, m, a, n - 11)
    w += [(f12 + 100, f10[2] - 50), (f12 + 500, f10[3] + 7)]
    nxt = _group(n, m, a + 1, n - 1 - 14)
    w += [(f10[3] + 20, nxt[1] + 300), (f10[2] - 1, nxt[3] + 1)]
    assert all(0 <= lo < hi <= total for lo, hi in w)
    return w


# (m, n, oracle): the root record alone and one real level, groups of 10 .. 20 selectable columns; several levels
SHAPES = [(7, 22, True), (8, 24, True), (12, 24, False), (16, 28, False)]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("m,n,oracle", SHAPES)
def test_whole_range_both_ways(ctx, monkeypatch, m, n, oracle, seed):
    A, b, c = _lp(m, n, 1500 + 10 * m + seed)
    got = _both_ways(ctx, monkeypatch, A, b, c, [(0, o.binom(n, m))], oracle)
    if oracle:
        assert got[0][0] == o.OPTIMAL and got[0][2][0] > 0


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("m,n", [(7, 22), (8, 24)])
def test_windows_inside_sub_groups_tails_and_packed_items(ctx, monkeypatch, m, n, seed):
    """passes clipped at either end: the windows of _windows, the oracle on the short ones"""
    A, b, c = _lp(m, n, 1500 + 10 * m + seed)
    windows = _windows(m, n)
    got = _both_ways(ctx, monkeypatch, A, b, c, windows)
    for w, g in zip(windows, got):
        if w[1] - w[0] <= 20000:
            assert g[:4] == _oracle(A, b, c, *w), w


MANY_SEED = 1583   # chosen on the CPU: 78,879 of the 735,471 subsets are feasible (10.7 %)


def _degenerate_vertex_lp(m, n, seed, j0=0, j1=9):
    """b = 0 on half of the rows, and a vertex that a tenth of all bases share: columns j0 and j1 are zero in the even
    rows and b is their sum, so every basis that holds both has x = 1 on them and 0 (to rounding) elsewhere — feasible.
    Below a prefix with both columns every lane of a pass survives; where j1 is one of the lanes' columns, some do."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, (m, n))
    A[::2, j0] = 0.0
    A[::2, j1] = 0.0
    return A, A[:, j0] + A[:, j1], rng.uniform(-1.0, 1.0, n)


def test_many_survivors_of_phase_one(ctx, monkeypatch):
    """b = 0 on half of the rows and a massively degenerate vertex: up to all 64 lanes of a pass survive phase 1, and
    phase 2 runs through every row of the tableau.  The feasible share (CPU oracle) lies above 1/16 and below a third,
    the dense form's threshold: the list form runs."""
    m, n = 8, 24
    A, b, c = _degenerate_vertex_lp(m, n, MANY_SEED)
    assert not b[::2].any() and b[1::2].all()
    total = o.binom(n, m)
    ref = _oracle(A, b, c, 0, total)
    assert total // 16 < ref[2][0] < total // 3, ref[2]
    windows = [(0, total)] + _windows(m, n)[1:8]
    got = _both_ways(ctx, monkeypatch, A, b, c, windows)
    assert got[0][:4] == ref


def _small_integer_lp(m, n, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-1, 2, size=(m, n)).astype(np.float64)
    b = rng.integers(1, 6, size=m).astype(np.float64)
    c = rng.integers(-3, 4, size=n).astype(np.float64)
    return A, b, c


@pytest.mark.parametrize("m,n,seed", [(7, 22, 91), (8, 24, 92)])
def test_exactly_singular_subsets(ctx, monkeypatch, m, n, seed):
    """small-integer data: thousands of subsets are singular by an exactly-zero pivot, in phase 1 of a 4-column pass
    or behind a shared pivot"""
    A, b, c = _small_integer_lp(m, n, seed)
    got = _both_ways(ctx, monkeypatch, A, b, c, [(0, o.binom(n, m))] + _windows(m, n)[1:6], oracle=(m == 7))
    assert got[0][2][2] > 2000


@pytest.mark.parametrize("scale", [2.0 ** -510, 2.0 ** 505])
@pytest.mark.parametrize("m,n,seed", [(7, 22, 1591), (8, 24, 1592)])
def test_pivots_outside_fast_reciprocal_range(ctx, monkeypatch, m, n, seed, scale):
    """A problem scaled so that every pivot lies outside the fast reciprocal's range: the pass raises the range flag
    and is repeated on the EXACT instantiations."""
    A, b, c = _lp(m, n, seed)
    A, b = A * scale, b * scale
    total = o.binom(n, m)
    ref = _oracle(A, b, c, 0, total)
    assert ref[2][0] > 0
    p = _problem(ctx, monkeypatch, A, b, c)
    assert not p.exact_division
    assert _result(p, 0, total, capi.ENUM_PREFIX)[:4] == ref
    assert p.exact_division
    p.free()
    windows = [(0, total)] + _windows(m, n)[1:8]
    _both_ways(ctx, monkeypatch, A, b, c, windows)
    _both_ways(ctx, monkeypatch, A, b, c, windows, LP_ENUM_EXACT_DIV=1)


def test_whole_range_three_times(ctx, monkeypatch):
    """the same whole range three times in a row: the direct kernel's counts every time"""
    m, n = 12, 24
    A, b, c = _lp(m, n, 1620)
    total = o.binom(n, m)
    p = _problem(ctx, monkeypatch, A, b, c)
    ref = p.range(0, total, capi.ENUM_DIRECT)[:3]
    assert sum(ref[2]) == total
    for _ in range(3):
        assert p.range(0, total, capi.ENUM_PREFIX)[:3] == ref
    p.free()
