"""GPU parity for the narrow depth m-7 nodes of the shared-prefix enumeration, which the last breadth-first level no
longer stores: k_enum_parent_tails (enum_leaf.hip) pivots them from the depth m-8 records and finishes their 1, 8 or 36
subsets.  Every comparison is bit for bit — status, optimum, tie-rule rank, the three counts and the winning vertex —
against the direct kernel, the same library with LP_ENUM_PARENT_TAILS=0 (every node stored, as before) and, where
the rank range is small enough for the CPU, the oracle."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from simplexmethod_amd import dist as lpdist
from tests import lpcases

pytestmark = pytest.mark.gpu

THIN_TAIL = 9   # enum_leaf.hip: a depth m-7 node with last column a >= n-1-THIN_TAIL is finished from its parent


def _problem(ctx, monkeypatch, A, b, c, tails=True, **env):
    """a problem whose knobs (read at upload) are LP_ENUM_PARENT_TAILS = tails (1: on whatever the size of the range,
    0: off; None: by the size of the range, as without the knob) and env"""
    with monkeypatch.context() as mp:
        mp.delenv("LP_ENUM_PARENT_TAILS", raising=False)
        if tails is not None:
            mp.setenv("LP_ENUM_PARENT_TAILS", "1" if tails else "0")
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
    """every window on the new path, the direct kernel, the stored-record path and (oracle=True) the CPU oracle"""
    on = _problem(ctx, monkeypatch, A, b, c, True, **env)
    got = [_result(on, lo, hi, capi.ENUM_PREFIX) for lo, hi in windows]
    direct = [_result(on, lo, hi, capi.ENUM_DIRECT) for lo, hi in windows]
    on.free()
    off = _problem(ctx, monkeypatch, A, b, c, False, **env)
    stored = [_result(off, lo, hi, capi.ENUM_PREFIX) for lo, hi in windows]
    off.free()
    for w, g, d, s in zip(windows, got, direct, stored):
        assert sum(g[2]) == w[1] - w[0], w
        assert g == d, (w, g[:4], d[:4])
        assert g == s, (w, g[:4], s[:4])
        if oracle:
            assert g[:4] == _oracle(A, b, c, *w), w
    return got


@functools.lru_cache(maxsize=None)
def _lp(m, n, seed):
    """random_lp is [dense | I]: an odd seed reverses the columns, so that the last ten — the narrow nodes' pivot and
    selectable columns — are the dense ones (the vertices and their count are the same)"""
    A, b, c, _ = lpcases.random_lp(seed, m, n)
    if seed % 2:
        A, c = np.ascontiguousarray(A[:, ::-1]), np.ascontiguousarray(c[::-1])
    for a in (A, b, c):
        a.setflags(write=False)
    return A, b, c


# (m, n): the parent is the root record; one real level in front; n - m = 7; every depth m-7 node is narrow (no stored
# record at all: the item builder, k_enum_thin and both leaf kernels see an empty level); parents with 0 .. 3 narrow
# children behind several wide levels (C(26,16): too many subsets for the CPU oracle)
SHAPES = [(8, 16, True), (9, 18, True), (10, 17, True), (14, 16, True), (12, 22, True), (16, 26, False)]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("m,n,oracle", SHAPES)
def test_whole_range_three_ways(ctx, monkeypatch, m, n, oracle, seed):
    A, b, c = _lp(m, n, 900 + 10 * m + seed)
    _three_ways(ctx, monkeypatch, A, b, c, [(0, o.binom(n, m))], oracle)


def _parent_end(n, m, prefix):
    """rank behind the last subset below the depth m-8 node `prefix` (m-8 ascending columns)"""
    rank, lo = 0, 0
    for k, col in enumerate(prefix):
        rank += sum(o.binom(n - 1 - q, m - 1 - k) for q in range(lo, col))
        lo = col + 1
    return rank + o.binom(n - lo, m - len(prefix))


def test_windows_inside_and_between_narrow_children(ctx, monkeypatch):
    """A parent's narrow children are its last 45 subsets, 36 | 8 | 1.  Windows that start and end inside the 36, on the
    seams between two children, at the parent's first and last subset, and across two parents; the second parent has
    two narrow children only (its last column is n-10)."""
    m, n = 12, 22
    A, b, c = _lp(m, n, 1021)
    windows = []
    for prefix in [(0, 1, 2, 3), (1, 3, 6, 9), (2, 5, 8, n - 10)]:
        e = _parent_end(n, m, prefix)
        first = e - o.binom(n - 1 - prefix[-1], 8)
        windows += [(e - 40, e - 20), (e - 45, e - 9), (e - 9, e - 1), (e - 10, e - 8), (e - 2, e), (e - 1, e), (e - 1, e + 1),
                    (e - 46, e - 44), (first, first + 1), (first, e), (e - 50, e + 50)]
    _three_ways(ctx, monkeypatch, A, b, c, windows)


def test_end_of_the_c32_16_rank_space(ctx, monkeypatch):
    """The last 4,000 ranks of C(32,16): parents with one, two and three narrow children and little else."""
    m, n = 16, 32
    A, b, c, _ = lpcases.random_lp(0, m, n)
    total = o.binom(n, m)
    got = _three_ways(ctx, monkeypatch, A, b, c, [(total - 4000, total), (total - 45, total), (total - 1, total)])
    assert got[0][2][0] > 0


def test_whole_c32_16_by_range_size(ctx, monkeypatch):
    """Without the knob the whole C(32,16), 2.04 M depth m-7 nodes, takes the new path (a small range does not):
    the same optimum, counts and tie-rule rank as with every node stored."""
    m, n = 16, 32
    A, b, c, _ = lpcases.random_lp(0, m, n)
    total = o.binom(n, m)
    out = []
    for tails in (None, False, True):
        p = _problem(ctx, monkeypatch, A, b, c, tails)
        out.append(_result(p, 0, total, capi.ENUM_PREFIX))
        p.free()
    assert out[0] == out[1] == out[2] and out[0][0] == o.OPTIMAL and sum(out[0][2]) == total


def test_cost_balanced_shards_compose(ctx, monkeypatch):
    m, n = 12, 22
    A, b, c = _lp(m, n, 1020)
    total = o.binom(n, m)
    whole = _oracle(A, b, c, 0, total)
    assert whole[0] == o.OPTIMAL
    cuts = [lpdist.balanced_shard_bounds(n, m, q, 8) for q in range(8)]
    assert cuts[0][0] == 0 and cuts[-1][1] == total
    parts = _three_ways(ctx, monkeypatch, A, b, c, cuts, oracle=False)
    assert max(r[1] for r in parts if r[0] == o.OPTIMAL) == whole[1]
    assert np.sum([r[2] for r in parts], axis=0).tolist() == whole[2]
    assert min(r[3] for r in parts if r[0] == o.OPTIMAL and r[1] == whole[1]) == whole[3]


def test_exactly_singular_child_pivots(ctx, monkeypatch):
    """Small integers: a zero column and a duplicate among the last ten make child pivots exactly zero — the subsets
    below them are counted singular without running, as the level kernel counts a hole."""
    m, n = 9, 19
    rng = np.random.default_rng(74)
    A = rng.integers(-1, 4, size=(m, n)).astype(np.float64)
    b = rng.integers(1, 6, size=m).astype(np.float64)
    c = rng.integers(-3, 4, size=n).astype(np.float64)
    A[:, n - 9] = 0.0
    A[:, n - 8] = A[:, n - 10]
    A[:, n - 2] = A[:, n - 5]
    total = o.binom(n, m)
    ref = _oracle(A, b, c, 0, total)
    assert ref[0] == o.OPTIMAL and ref[2][2] > 1000
    got = _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (total - 3000, total - 2)])
    assert got[0][2][2] == ref[2][2]


def test_nan_and_inf_in_the_last_columns(ctx, monkeypatch):
    m, n = 9, 19
    A, b, c = (a.copy() for a in _lp(m, n, 1035))
    A[2, n - 8] = np.nan
    A[5, n - 10] = np.inf
    A[0, n - 9] = -np.inf
    A[7, n - 3] = np.nan
    total = o.binom(n, m)
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (total - 500, total)])


def test_child_pivot_at_the_singularity_threshold(ctx, monkeypatch):
    """Column 0 is a unit vector, so the node {0} has min = max = 1; the largest entry of column n-9 in the other rows
    is eps * m exactly (the child is pruned: min <= eps * m * max) and that of column n-8 the next double above it."""
    m, n = 9, 18
    A, b, c = (a.copy() for a in _lp(m, n, 1033))
    A[:, 0] = 0.0
    A[0, 0] = 1.0
    t = np.finfo(np.float64).eps * m
    for col, top in ((n - 9, t), (n - 8, np.nextafter(t, 1.0))):
        A[1:, col] *= 0.25 * top / np.abs(A[1:, col]).max()
        A[4, col] = top
    total = o.binom(n, m)
    ref = _oracle(A, b, c, 0, total)
    assert ref[2][2] > 0
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (0, o.binom(n - 1, m - 1))])


@pytest.mark.parametrize("m,n,seed", [(8, 16, 1040), (9, 18, 1041), (12, 22, 1042)])
def test_plain_division_agrees(ctx, monkeypatch, m, n, seed):
    A, b, c = _lp(m, n, seed)
    total = o.binom(n, m)
    fast = _three_ways(ctx, monkeypatch, A, b, c, [(0, total)])
    p = _problem(ctx, monkeypatch, A, b, c, True, LP_ENUM_EXACT_DIV=1)
    assert _result(p, 0, total, capi.ENUM_PREFIX) == fast[0] and p.exact_division
    p.free()


@pytest.mark.parametrize("m,n,seed", [(8, 16, 1050), (9, 18, 1051)])
def test_scaled_problem_raises_the_range_flag(ctx, monkeypatch, m, n, seed):
    """Scaled by 2^-510 every pivot lies outside the fast reciprocal's range.  The last 8 ranks lie below narrow nodes
    only, so the flag is k_enum_parent_tails' own and the pass is repeated on its EXACT instantiation."""
    A, b, c = _lp(m, n, seed)
    A, b = A * 2.0 ** -510, b * 2.0 ** -510
    total = o.binom(n, m)
    ref = _oracle(A, b, c, total - 8, total)
    p = _problem(ctx, monkeypatch, A, b, c, True)
    assert not p.exact_division
    assert _result(p, total - 8, total, capi.ENUM_PREFIX)[:4] == ref
    assert p.exact_division
    assert _result(p, 0, total, capi.ENUM_PREFIX)[:4] == _oracle(A, b, c, 0, total)
    p.free()
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total), (total - 8, total)])


def _narrow_windows(n, m):
    """the rank windows of every depth m-8 node's narrow children (m = 9: the nodes are the single columns)"""
    assert m == 9
    out = []
    for a0 in range(n - m + 1):
        e = _parent_end(n, m, (a0,))
        cnt = min(o.binom(n - 1 - a0, 8), 45)
        out.append((e - cnt, e))
    return out


def test_feasible_entries_without_a_record(ctx, monkeypatch):
    """b = 0 on half of the rows: many feasible bases, a list of 300 entries to start with.  Feasible subsets below a
    narrow node have no depth m-7 record and are scored from scratch; the optimum and the tie-rule winner must be the
    direct kernel's — on the whole range and on windows that hold narrow nodes only."""
    m, n = 9, 18
    A, b, c = (a.copy() for a in _lp(m, n, 1060))
    b[::2] = 0.0
    total = o.binom(n, m)
    windows = _narrow_windows(n, m)
    # CPU: at least one feasible subset whose (m-7)-th smallest column is at or beyond n-1-THIN_TAIL
    feas = [o.enum_range(A, b, c, True, lo, hi)[2][0] for lo, hi in windows]
    assert sum(feas) > 0 and o.enum_range(A, b, c, True, 0, total)[2][0] > 300
    busy = [w for w, f in zip(windows, feas) if f > 0]
    _three_ways(ctx, monkeypatch, A, b, c, [(0, total)] + busy, LP_ENUM_LIST_START=300)


def test_fully_degenerate_goes_dense(ctx, monkeypatch):
    """b = 0: every non-singular basis is feasible; the pass goes to the dense form, where every node is stored."""
    m, n = 9, 18
    A, b, c = (a.copy() for a in _lp(m, n, 1062))
    b[:] = 0.0
    _three_ways(ctx, monkeypatch, A, b, c, [(0, o.binom(n, m))], LP_ENUM_LIST_START=300)


def test_repetition_gives_identical_counts(ctx, monkeypatch):
    m, n = 12, 22
    A, b, c = _lp(m, n, 1020)
    total = o.binom(n, m)
    lo, hi = total // 7 + 5, total - total // 11
    ref = _oracle(A, b, c, lo, hi)
    p = _problem(ctx, monkeypatch, A, b, c, True)
    for _ in range(20):
        rc, z, counts, _ = p.range(lo, hi, capi.ENUM_PREFIX)
        assert (rc, z, counts) == ref[:3]   # (counts[0] is the length of the feasible list)
    p.free()


def test_last_level_in_its_narrow_form(ctx, monkeypatch):
    """LP_ENUM_NARROW_MULT: every level as one wave per child (k_enum_expand_narrow), or none (k_enum_expand_staged)."""
    m, n = 12, 22
    A, b, c = _lp(m, n, 1020)
    total = o.binom(n, m)
    windows = [(0, total), (total // 3, total // 3 + 70000)]
    staged = _three_ways(ctx, monkeypatch, A, b, c, windows, oracle=False, LP_ENUM_NARROW_MULT=0)
    narrow = _three_ways(ctx, monkeypatch, A, b, c, windows, oracle=False, LP_ENUM_NARROW_MULT=1 << 20)
    assert staged == narrow
    assert staged[0][:4] == _oracle(A, b, c, 0, total)
