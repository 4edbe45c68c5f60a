"""GPU parity for the head of the leaf kernels' passes (k_enum_leaves<3> and <0> in enum_leaf.hip): the subset-table word
is loaded one pass ahead with a clamped index, and the loop bounds of a sub-group, a group's 5-column tail and an m = 6
chunk are cut to the rank window once instead of every lane testing its rank.  The shared-prefix path against the direct
kernel and the oracle — status, optimum, counts and tie-rule rank, bit for bit — on rank windows that begin and end on,
just before and just behind a pass boundary of a sub-group or a tail, windows of a few subsets, windows that end inside
a part-filled last pass, random windows, both item widths, the EXACT instantiations, both table-0 kernels and m = 6.
The cases that need no GPU (a window against its two halves, the layout the windows are built from) run on the oracle."""
import contextlib
import functools

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import lpcases

WINDOW = 300000     # a rank space is cut to its first WINDOW ranks
GREAT_MIN = 9       # enum_leaf.hip kGreatMin: a sub-group has at least 9 selectable columns, the rest is the group's tail
TAIL = o.binom(GREAT_MIN, 5)   # ... the group's last 126 subsets: two 5-column passes

# seeds of tests/test_gpu_enum_leaf_steps.py that have feasible subsets among the first WINDOW ranks
SHAPES = [(7, 23, 986), (8, 22, 994), (9, 21, 1002)]


@functools.lru_cache(maxsize=None)
def _lp(m, n, seed, kind="random"):
    if kind == "random":
        A, b, c, _ = lpcases.random_lp(seed, m, n)
    else:   # entries in -2 .. 2, a third of them zero (tests/test_gpu_enum_leaf_steps.py: test_exact_ties_and_zeros)
        rng = np.random.default_rng(seed)
        A = rng.integers(-2, 3, (m, n)).astype(float)
        A[rng.random((m, n)) < 0.35] = 0.0
        b = rng.integers(0, 4, m).astype(float)
        c = rng.integers(-2, 4, n).astype(float)
    for a in (A, b, c):
        a.setflags(write=False)
    return A, b, c, min(o.binom(n, m), WINDOW)


@functools.lru_cache(maxsize=None)
def _whole(m, n, seed, kind="random"):
    """the oracle over [0, hi): ((status, optimum, counts), tie-rule rank); computed once, read-only"""
    A, b, c, hi = _lp(m, n, seed, kind)
    ref = o.enum_range(A, b, c, True, 0, hi)
    assert ref[0] == o.OPTIMAL and ref[2][0] > 0
    return ref, o.enum_first_within(A, b, c, True, 0, hi, ref[1])


def _oracle(A, b, c, lo, up):
    st, z, counts = o.enum_range(A, b, c, True, lo, up)
    return st, z, counts, (o.enum_first_within(A, b, c, True, lo, up, z) if st == o.OPTIMAL else None)


def _first_rank(n, m, prefix):
    """rank of the first m-subset (lexicographic order) whose first columns are `prefix` (ascending)"""
    rank, prev = 0, -1
    for i, col in enumerate(prefix):
        rank += sum(o.binom(n - 1 - q, m - 1 - i) for q in range(prev + 1, col))
        prev = col
    return rank


def _below(n, m, prefix):
    """number of m-subsets that begin with `prefix`"""
    return o.binom(n - 1 - prefix[-1], m - len(prefix))


def _sub_groups(m, n):
    """(first rank, size) of three sub-groups — prefixes of m - 4 columns: the record's m - 7, the child's, the group's
    and the sub-group's — all inside [0, WINDOW): the very first, one behind skipped columns at every shared pivot, and
    the narrowest the first group has (9 selectable columns, 126 subsets: one full pass and a part-filled one)"""
    k = m - 4
    first = tuple(range(k))
    skipped = tuple(range(k - 3)) + (k - 2, k, k + 2)
    narrow = tuple(range(k - 1)) + (n - 1 - GREAT_MIN,)
    out = [(_first_rank(n, m, p), _below(n, m, p)) for p in (first, skipped, narrow)]
    assert out[2][1] == TAIL and all(s >= TAIL and g + s <= min(o.binom(n, m), WINDOW) for g, s in out)
    return out


def _tails(m, n):
    """(first rank of the group, first rank of its 5-column tail, rank behind it) of two groups (prefixes of m - 5)"""
    k = m - 5
    out = []
    for p in (tuple(range(k)), tuple(range(k - 2)) + (k - 1, k + 2)):
        g, size = _first_rank(n, m, p), _below(n, m, p)
        assert size > 2 * TAIL and g + size <= min(o.binom(n, m), WINDOW)
        out.append((g, g + size - TAIL, g + size))
    return out


def _pass_head_windows(m, n):
    """the rank windows of one shape, around the passes of its sub-groups and tails"""
    ws = []
    for g, size in _sub_groups(m, n):
        last = g + 64 * ((size - 1) // 64)           # first subset of the sub-group's last pass
        assert size % 64 not in (0, 1), "the last pass is part-filled"
        for d in (-1, 0, 1):
            ws.append((g + 64 + d, g + size))         # begins on / before / behind a pass boundary
            ws.append((g, g + 64 + d))                # ends there
            ws.append((g + 64 + d, g + 128 - d))
            ws.append((g + d if g + d >= 0 else 0, last + 1 + d if d >= 0 else last))   # ends in / at the last pass
        for w in (1, 63, 64, 65, 129):
            for at in (g, g + 64, g + 70, g + size - w):
                if at + w <= g + size:
                    ws.append((at, at + w))
        ws += [(g, last + 1), (g, g + size - 1), (g + 7, g + size - 1), (last, g + size - 1), (last + 1, g + size),
               (g + size - 1, g + size + 1)]
    for g, t, e in _tails(m, n):
        ws += [(t - 1, t + 1), (t, t + 64), (t + 1, e), (t + 63, e), (t + 64, t + 65), (t + 64, e - 1), (g, t + 65),
               (t - 70, t + 63), (t + 5, e - 5), (e - 1, e + 1)]
    assert all(0 <= lo < up <= min(o.binom(n, m), WINDOW) for lo, up in ws)
    return sorted(set(ws))


def _random_windows(m, n, count=24):
    rng = np.random.default_rng(7000 + 100 * m + n)
    hi = min(o.binom(n, m), WINDOW)
    ws = []
    for _ in range(count):
        w = int(2 ** rng.uniform(0, 14))              # 1 .. 16 k subsets
        lo = int(rng.integers(0, hi - w))
        ws.append((lo, lo + w))
    return ws


@contextlib.contextmanager
def _problem(ctx, monkeypatch, A, b, c, **env):
    """an uploaded problem whose knobs (read at upload) are `env`; freed also when an assertion fails"""
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, str(v))
        p = ctx.enum_problem(A, b, c, True)
    try:
        yield p
    finally:
        p.free()


def _both(p, lo, up):
    """(status, optimum, counts, tie-rule rank) of [lo, up) on the shared-prefix path; the direct kernel must agree"""
    out = []
    for algo in (capi.ENUM_PREFIX, capi.ENUM_DIRECT):
        rc, z, counts, _ = p.range(lo, up, algo)
        out.append((rc, z, counts, p.first_within(lo, up, z) if rc == o.OPTIMAL else None))
    assert out[0] == out[1], (lo, up, out)
    assert sum(out[0][2]) == up - lo, (lo, up)
    return out[0]


def _check_windows(p, A, b, c, windows):
    for lo, up in windows:
        assert _both(p, lo, up) == _oracle(A, b, c, lo, up), (lo, up)


# ---- without a GPU: the layout the windows are built from, and a window against its halves on the oracle

@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_window_layout_cpu(m, n, seed):
    """the sub-groups and tails are where the ranks say: the subset at a first rank begins with the prefix, the one
    in front of it does not (checked by unranking on the CPU)"""
    def unrank(rank):
        cols, col = [], 0
        for i in range(m):
            while rank >= o.binom(n - 1 - col, m - 1 - i):
                rank -= o.binom(n - 1 - col, m - 1 - i)
                col += 1
            cols.append(col)
            col += 1
        return tuple(cols)
    k = m - 4
    for p in (tuple(range(k)), tuple(range(k - 3)) + (k - 2, k, k + 2), tuple(range(k - 1)) + (n - 1 - GREAT_MIN,)):
        g = _first_rank(n, m, p)
        assert unrank(g)[:k] == p and unrank(g + _below(n, m, p) - 1)[:k] == p
        assert g == 0 or unrank(g - 1)[:k] != p
    assert len(_pass_head_windows(m, n)) > 100


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_windows_add_up_cpu(m, n, seed):
    """oracle alone: a window's counts are the sum of its halves', its optimum the better half's — for the windows cut
    in the middle of a pass that the GPU tests use"""
    A, b, c, _ = _lp(m, n, seed)
    ws = [w for w in _pass_head_windows(m, n) if w[1] - w[0] >= 2][::6] + _random_windows(m, n, 8)
    for lo, up in ws:
        mid = lo + (up - lo) // 2 + (1 if (up - lo) > 64 else 0)
        whole, left, right = (o.enum_range(A, b, c, True, x, y) for x, y in ((lo, up), (lo, mid), (mid, up)))
        assert whole[2] == [l + r for l, r in zip(left[2], right[2])], (lo, up)
        zs = [h[1] for h in (left, right) if h[0] == o.OPTIMAL]
        assert (whole[0] == o.OPTIMAL) == bool(zs) and (not zs or whole[1] == max(zs)), (lo, up)


# ---- on the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_whole_range_and_pass_head_windows(ctx, monkeypatch, m, n, seed):
    A, b, c, hi = _lp(m, n, seed)
    ref, k = _whole(m, n, seed)
    with _problem(ctx, monkeypatch, A, b, c) as p:
        assert _both(p, 0, hi) == (ref[0], ref[1], ref[2], k)
        _check_windows(p, A, b, c, _pass_head_windows(m, n))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_random_windows(ctx, monkeypatch, m, n, seed):
    A, b, c, _ = _lp(m, n, seed)
    with _problem(ctx, monkeypatch, A, b, c) as p:
        _check_windows(p, A, b, c, _random_windows(m, n))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_windows_and_their_halves(ctx, monkeypatch, m, n, seed):
    """a window cut in the middle of a pass: the two pieces' counts add up to the window's on the shared-prefix path"""
    A, b, c, _ = _lp(m, n, seed)
    with _problem(ctx, monkeypatch, A, b, c) as p:
        for lo, up in [w for w in _pass_head_windows(m, n) if w[1] - w[0] >= 2][::6]:
            mid = lo + (up - lo) // 2 + (1 if (up - lo) > 64 else 0)
            whole, left, right = (p.range(x, y, capi.ENUM_PREFIX) for x, y in ((lo, up), (lo, mid), (mid, up)))
            assert list(whole[2]) == [l + r for l, r in zip(left[2], right[2])], (lo, up)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1024, 2048])
def test_item_widths(ctx, monkeypatch, chunk):
    """LP_ENUM_CHUNK: a chunk boundary inside a group moves the first leaf of the loops (and with it the passes)"""
    m, n, seed = SHAPES[0]
    A, b, c, hi = _lp(m, n, seed)
    ref, k = _whole(m, n, seed)
    g, size = _first_rank(n, m, (0, 0 + 1)), _below(n, m, (0, 1))
    assert size > 2 * 2048
    t = g + size - TAIL
    windows = [(g + chunk - 1, g + chunk + 65), (g + chunk, g + chunk + 64), (g + chunk + 1, g + 2 * chunk - 1),
               (g + chunk - 70, g + chunk + 129), (g + 1000, t + 70), (t - chunk, t + 1), (g + 2 * chunk + 1, g + size)]
    with _problem(ctx, monkeypatch, A, b, c, LP_ENUM_CHUNK=chunk) as p:
        assert _both(p, 0, hi) == (ref[0], ref[1], ref[2], k)
        _check_windows(p, A, b, c, windows + _pass_head_windows(m, n)[::5])


@pytest.mark.gpu
def test_exact_ties_and_zeros(ctx, monkeypatch):
    """integer entries: whole sub-groups are singular at the shared pivot (counted through the clamped window), ties at
    every step; the pass must not go to the plain divisions"""
    m, n, seed = 8, 19, 42
    A, b, c, hi = _lp(m, n, seed, "integer")
    ref, k = _whole(m, n, seed, "integer")
    assert ref[2][2] > 1000
    with _problem(ctx, monkeypatch, A, b, c) as p:
        assert _both(p, 0, hi) == (ref[0], ref[1], ref[2], k)
        _check_windows(p, A, b, c, _pass_head_windows(m, n)[::4] + _random_windows(m, n, 8))
        assert not p.exact_division


@pytest.mark.gpu
def test_scaled_problem_runs_the_exact_loops(ctx, monkeypatch):
    """scaled by 1e-160: the pivots leave the fast reciprocal's range, the pass raises the redo flag and is repeated
    on the EXACT instantiations, whose loops have the same head"""
    m, n, seed = SHAPES[1]
    A, b, c, hi = _lp(m, n, seed)
    A, b = A * 1e-160, b * 1e-160
    ref = _oracle(A, b, c, 0, hi)
    assert ref[0] == o.OPTIMAL and ref[2][0] > 0
    windows = _pass_head_windows(m, n)[::4] + _random_windows(m, n, 8)
    with _problem(ctx, monkeypatch, A, b, c) as p:
        assert not p.exact_division
        assert _both(p, 0, hi) == ref
        assert p.exact_division
        _check_windows(p, A, b, c, windows)
    with _problem(ctx, monkeypatch, A, b, c, LP_ENUM_EXACT_DIV=1) as p:
        _check_windows(p, A, b, c, windows[::3])


@pytest.mark.gpu
@pytest.mark.parametrize("quads", [0, 1])
def test_both_table0_kernels(ctx, monkeypatch, quads):
    """m = 7, n = 17: the root's children have 16 .. 9 selectable columns, the children of 9 and 10 among them;
    k_enum_leaves_quads and k_enum_leaves<1> finish table 0 and agree with the direct kernel and the oracle"""
    m, n, seed = 7, 17, 977
    A, b, c, hi = _lp(m, n, seed)
    assert hi == o.binom(n, m)
    nine, ten = _first_rank(n, m, (n - 10,)), _first_rank(n, m, (n - 11,))   # children with 9 and 10 selectable columns
    assert _below(n, m, (n - 10,)) == o.binom(9, 6) and _below(n, m, (n - 11,)) == o.binom(10, 6)
    windows = [(0, hi), (ten, nine), (ten - 1, ten + 65), (ten + 64, nine + 1), (nine, nine + 84), (nine + 1, nine + 64),
               (ten + 63, nine + 65), (nine - 1, hi)]
    with _problem(ctx, monkeypatch, A, b, c, LP_ENUM_LEAF_QUADS=quads) as p:
        _check_windows(p, A, b, c, windows + _random_windows(m, n, 8))


@pytest.mark.gpu
def test_m6_chunks(ctx, monkeypatch):
    """m = 6 (k_enum_leaves<0>): the root is the record, chunks of 1024 subsets; windows around the chunk and pass
    boundaries and inside the last, part-filled pass of the last chunk"""
    m, n, seed = 6, 22, 961
    A, b, c, hi = _lp(m, n, seed)
    assert hi == o.binom(n, m) and hi % 1024 % 64 not in (0, 1)
    last = 1024 * (hi // 1024) + 64 * ((hi % 1024 - 1) // 64)
    windows = [(0, hi), (0, 1), (63, 65), (64, 128), (65, 1024), (1023, 1025), (1024, 1088), (1025, 1024 + 129),
               (1000, 3000), (last, hi), (last + 1, hi - 1), (last - 1, last + 1), (0, hi - 1), (2048 + 64, last + 1),
               (hi - 1, hi)]
    with _problem(ctx, monkeypatch, A, b, c) as p:
        _check_windows(p, A, b, c, windows + _random_windows(m, n, 12))
