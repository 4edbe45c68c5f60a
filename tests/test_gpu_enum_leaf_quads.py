"""GPU parity for table 0 of the shared-prefix enumeration finished by k_enum_leaves_quads (enum_leaf.hip): one table
entry per depth m-6 child, four children pivoted per wave at once from registers, passes of 64 subsets that run on
from one round of children into the next.  Every comparison is bit for bit — status, optimum, tie-rule rank, the three
counts and the winning vertex — against the direct kernel, the same library with LP_ENUM_LEAF_QUADS=0 (k_enum_leaves<1>
on paired items) and, where the rank range is small enough for the CPU, the oracle."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import lpcases

pytestmark = pytest.mark.gpu

GRAND_MIN = 10   # enum_leaf.hip kGrandMin: a child's table-0 tail are its subsets inside its last 10 selectable columns
THIN_TAIL = 9    # ... and only children with at least 9 selectable columns are in table 0


def _problem(ctx, monkeypatch, A, b, c, quads=True, **env):
    """a problem whose knobs (read at upload) are LP_ENUM_LEAF_QUADS = quads (None: unset) and env"""
    with monkeypatch.context() as mp:
        mp.delenv("LP_ENUM_LEAF_QUADS", raising=False)
        if quads is not None:
            mp.setenv("LP_ENUM_LEAF_QUADS", "1" if quads else "0")
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


def _three_ways(ctx, monkeypatch, A, b, c, windows, oracle=True, **env):
    """every window on the new kernel, the direct kernel, the paired-item kernel and (oracle=True) the CPU oracle"""
    on = _problem(ctx, monkeypatch, A, b, c, True, **env)
    got = [_result(on, lo, hi, capi.ENUM_PREFIX) for lo, hi in windows]
    direct = [_result(on, lo, hi, capi.ENUM_DIRECT) for lo, hi in windows]
    on.free()
    off = _problem(ctx, monkeypatch, A, b, c, False, **env)
    paired = [_result(off, lo, hi, capi.ENUM_PREFIX) for lo, hi in windows]
    off.free()
    for w, g, d, s in zip(windows, got, direct, paired):
        assert sum(g[2]) == w[1] - w[0], w
        assert g == d, (w, g[:4], d[:4])
        assert g == s, (w, g[:4], s[:4])
        if oracle:
            assert g[:4] == _oracle(A, b, c, *w), w
    return got


@functools.lru_cache(maxsize=None)
def _lp(m, n, seed):
    """random_lp is [dense | I]: an odd seed reverses the columns, so that the last ones — the columns the table-0
    tails choose from — are the dense ones (the vertices and their count are the same)"""
    A, b, c, _ = lpcases.random_lp(seed, m, n)
    if seed % 2:
        A, c = np.ascontiguousarray(A[:, ::-1]), np.ascontiguousarray(c[::-1])
    for a in (A, b, c):
        a.setflags(write=False)
    return A, b, c


# (m, n, oracle): the root is the only record, nine children (rounds of 4 + 4 + 1); one and two real levels; several
# wide levels, records with a single 84-subset child packed across records; sixteen rows (too many subsets for the CPU)
SHAPES = [(7, 18, True), (8, 20, True), (9, 21, True), (12, 24, False), (16, 28, False)]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("m,n,oracle", SHAPES)
def test_whole_range_three_ways(ctx, monkeypatch, m, n, oracle, seed):
    A, b, c = _lp(m, n, 1200 + 10 * m + seed)
    _three_ways(ctx, monkeypatch, A, b, c, [(0, o.binom(n, m))], oracle)


def _node_end(n, m, prefix):
    """rank behind the last subset below the node `prefix` (ascending columns)"""
    rank, lo = 0, 0
    for k, col in enumerate(prefix):
        rank += sum(o.binom(n - 1 - q, m - 1 - k) for q in range(lo, col))
        lo = col + 1
    return rank + o.binom(n - lo, m - len(prefix))


def _tail(n, m, child):
    """[first, end) of the table-0 tail of the depth m-6 node `child`: its subsets inside its last 10 columns"""
    R = n - 1 - child[-1]
    assert len(child) == m - 6 and R >= THIN_TAIL
    e = _node_end(n, m, child)
    return e - o.binom(min(R, GRAND_MIN), 6), e


def test_windows_inside_and_between_tails(ctx, monkeypatch):
    """(12, 24): records are 5 columns, table-0 children end in columns <= 14; the child on column 14 has an 84-subset
    tail (all of it), the others 210."""
    m, n = 12, 24
    A, b, c = _lp(m, n, 1321)
    windows = []
    rec = (0, 1, 2, 3, 4)
    f84, e84 = _tail(n, m, rec + (14,))
    f210, e210 = _tail(n, m, rec + (13,))
    assert e84 - f84 == 84 and e210 - f210 == 210 and e210 == f84
    # start and end inside an 84-subset tail and inside a 210-subset tail; one subset only
    windows += [(f84 + 3, f84 + 70), (f84 + 20, f84 + 21), (f210 + 5, f210 + 140), (f210 + 64, f210 + 128),
                (f210, f210 + 1), (e210 - 1, e210), (e84 - 1, e84)]
    # exactly on the seam between two children of one record, and across it
    windows += [(f210, e210), (f84, e84), (f210 + 100, e84 - 10), (e210 - 1, e210 + 1)]
    # the seam between the last table-0 child of one record and the first of the next (0,1,2,3,5): its child on column 6
    nf, ne = _tail(n, m, (0, 1, 2, 3, 5, 6))
    windows += [(e84 - 30, nf + 30), (e84, nf + 1), (e84 - 1, ne)]
    # a record with a single 84-subset child (last column n - 11), and the record behind it
    sf, se = _tail(n, m, (0, 1, 2, 3, 13, 14))
    windows += [(sf, se), (sf + 80, se + 5000), (sf - 1, sf + 1)]
    # one, two or three of four consecutive children outside the range: windows that begin at the tail of the 2nd,
    # 3rd, 4th of the children on columns 11 .. 14 and end with the record, or begin in front and end before them
    first11 = _tail(n, m, rec + (11,))[0]
    for a in (12, 13, 14):
        ta = _tail(n, m, rec + (a,))[0]
        windows += [(ta, e84), (first11, ta), (first11 + 7, ta + 9)]
    _three_ways(ctx, monkeypatch, A, b, c, windows)


def test_shards_compose(ctx, monkeypatch):
    m, n = 12, 24
    A, b, c = _lp(m, n, 1320)
    total = o.binom(n, m)
    cuts = [0, total // 9, total // 3 + 17, total // 2, total - 100000, total - 1000, total]
    parts = _three_ways(ctx, monkeypatch, A, b, c, list(zip(cuts[:-1], cuts[1:])), oracle=False)
    whole = _three_ways(ctx, monkeypatch, A, b, c, [(0, total)], oracle=False)[0]
    assert np.sum([r[2] for r in parts], axis=0).tolist() == list(whole[2])
    assert max(r[1] for r in parts if r[0] == o.OPTIMAL) == whole[1]
    assert min(r[3] for r in parts if r[0] == o.OPTIMAL and r[1] == whole[1]) == whole[3]


def _small_integer_lp(m, n, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-1, 4, size=(m, n)).astype(np.float64)
    b = rng.integers(1, 6, size=m).astype(np.float64)
    c = rng.integers(-3, 4, size=n).astype(np.float64)
    return A, b, c


def test_zero_child_column(ctx, monkeypatch):
    """(9, 21): records are 2 columns, table-0 children end in columns 2 .. 11.  Column 8 is zero: every child on it is
    pruned, its subsets inside the range counted singular once."""
    m, n = 9, 21
    A, b, c = _small_integer_lp(m, n, 81)
    A[:, 8] = 0.0
    total = o.binom(n, m)
    f, e = _tail(n, m, (0, 1, 8))
    got = _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (f, e), (f + 10, e - 10), (f - 300, e + 300)])
    assert got[1][2] == [0, 0, 210] and got[2][2] == [0, 0, 190]


def test_child_column_equal_to_column_zero(ctx, monkeypatch):
    """Column 9 equals column 0: the child on 9 is pruned under the records that contain column 0 only, so pruned and
    live children share rounds."""
    m, n = 9, 21
    A, b, c = _small_integer_lp(m, n, 82)
    A[:, 9] = A[:, 0]
    total = o.binom(n, m)
    f, e = _tail(n, m, (0, 3, 9))
    g, h = _tail(n, m, (1, 3, 9))
    got = _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (f, e), (g, h), (f - 500, e + 500)])
    assert got[1][2] == [0, 0, 210] and got[2][2][2] < 210


def test_table_zero_all_singular(ctx, monkeypatch):
    """Columns 2 .. 11 are zero: every record but (0, 1) that could have a table-0 child is a hole, and every child of
    (0, 1) is pruned."""
    m, n = 9, 21
    A, b, c = _small_integer_lp(m, n, 83)
    A[:, 2:12] = 0.0
    total = o.binom(n, m)
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (0, _node_end(n, m, (0, 1)))])


@pytest.mark.parametrize("m,n", [(9, 21), (12, 24)])
def test_level_with_pruned_records(ctx, monkeypatch, m, n):
    """Repeated, proportional and zero columns: holes in the levels, pruned children beside live ones."""
    A, b, c, _ = lpcases.random_lp(1400 + n, m, n)
    A[:, 1] = A[:, 0]
    A[:, m - 3] = 3.0 * A[:, m - 5]
    A[:, n // 2] = 0.0
    A[:, n - 2] = A[:, n - 5]
    total = o.binom(n, m)
    cuts = [0, total // 7, total // 3, total // 2 + 11, total - 1000, total]
    got = _three_ways(ctx, monkeypatch, A, b, c, [(0, total)] + list(zip(cuts[:-1], cuts[1:])), oracle=(m == 9))
    assert got[0][2][2] > total // 4


@pytest.mark.parametrize("m,n,seed", [(7, 18, 1440), (9, 21, 1441), (12, 24, 1442)])
def test_plain_division_agrees(ctx, monkeypatch, m, n, seed):
    A, b, c = _lp(m, n, seed)
    total = o.binom(n, m)
    fast = _three_ways(ctx, monkeypatch, A, b, c, [(0, total)], oracle=False)
    p = _problem(ctx, monkeypatch, A, b, c, True, LP_ENUM_EXACT_DIV=1)
    assert _result(p, 0, total, capi.ENUM_PREFIX) == fast[0] and p.exact_division
    p.free()
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total)], oracle=False, LP_ENUM_EXACT_DIV=1)


@pytest.mark.parametrize("m,n,seed", [(7, 18, 1450), (9, 21, 1451)])
def test_scaled_problem_raises_the_range_flag(ctx, monkeypatch, m, n, seed):
    """Scaled by 2^-510 every pivot lies outside the fast reciprocal's range.  The window lies inside one table-0 tail,
    so the flag is this kernel's own and the pass is repeated on its EXACT instantiation."""
    A, b, c = _lp(m, n, seed)
    A, b = A * 2.0 ** -510, b * 2.0 ** -510
    total = o.binom(n, m)
    f, e = _tail(n, m, tuple(range(m - 6)))
    lo, hi = f + 50, e - 50
    ref = _oracle(A, b, c, lo, hi)
    p = _problem(ctx, monkeypatch, A, b, c, True)
    assert not p.exact_division
    assert _result(p, lo, hi, capi.ENUM_PREFIX)[:4] == ref
    assert p.exact_division
    p.free()
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (lo, hi)])


def test_list_overflow_and_dense_switch(ctx, monkeypatch):
    """b = 0 on half of the rows, then on all: a list of 300 entries to start with grows, or gives way to the dense form."""
    m, n = 9, 21
    A, b, c = (a.copy() for a in _lp(m, n, 1460))
    b[::2] = 0.0
    total = o.binom(n, m)
    f, e = _tail(n, m, (0, 1, 2))
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (f, e)], LP_ENUM_LIST_START=300)
    b[:] = 0.0
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total)], LP_ENUM_LIST_START=300)


def test_repetition_deals_every_entry_once(ctx, monkeypatch):
    """The same whole range 20 times: the three counts are the direct kernel's every time — no entry is lost or done
    twice at the end of the table, however the runs fall."""
    m, n = 12, 24
    A, b, c = _lp(m, n, 1320)
    total = o.binom(n, m)
    p = _problem(ctx, monkeypatch, A, b, c, True)
    ref = p.range(0, total, capi.ENUM_DIRECT)[:3]
    assert sum(ref[2]) == total
    for _ in range(20):
        assert p.range(0, total, capi.ENUM_PREFIX)[:3] == ref
    p.free()


def test_unset_knob_is_the_new_kernel_or_the_old(ctx, monkeypatch):
    """Without the knob: the same answers as with either setting."""
    m, n = 12, 24
    A, b, c = _lp(m, n, 1322)
    total = o.binom(n, m)
    out = []
    for quads in (None, False, True):
        p = _problem(ctx, monkeypatch, A, b, c, quads)
        out.append(_result(p, 0, total, capi.ENUM_PREFIX))
        p.free()
    assert out[0] == out[1] == out[2] and sum(out[0][2]) == total
