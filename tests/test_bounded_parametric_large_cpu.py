"""What the cases of tests/bounded_parametric_large_cases.py exercise, asserted on the reference alone (no GPU), so that
tests/test_gpu_bounded_parametric_large.py cannot quietly lose coverage: the statuses, the bound flips, the leaves at an
upper bound and the zero-length segments of the cases beyond one workgroup's LDS, the convexity of their slopes, and on
the 1100 x 2300 cases the exact ties across the 1024 seam with their winners, positions and columns beyond 1024."""
import numpy as np
import pytest

from tests import bounded_parametric_large_cases as L

OPTIMAL, UNBOUNDED, ITER_LIMIT, INFEASIBLE = L.OPTIMAL, L.UNBOUNDED, L.ITER_LIMIT, L.INFEASIBLE


def _path(r):
    ns = r["nseg"]
    return ns, r["t"][:ns + 1], r["slope"][:ns], r["enter"][:ns], r["leave"][:ns], r["side"][:ns]


def _zero_length(t, ns):
    return int((np.diff(t[:ns]) == 0.0).sum())   # segments k < ns - 1 with t[k + 1] == t[k]


@pytest.mark.parametrize("key", L.BEYOND, ids=L.key_id)
def test_beyond_cases_exercise_the_box(key):
    path, m, n, seed, maximize, kind = key
    cs = L.beyond(*key)
    r = L.ref(L.key_id(key), path, cs)
    ns, t, slope, enter, leave, side = _path(r)
    want = ITER_LIMIT if key == L.LIMIT else UNBOUNDED if key == L.RAY else INFEASIBLE if path == "rhs" else OPTIMAL
    assert r["status"] == want
    assert ns > 40 and (key == L.LIMIT) == (ns == L.BEYOND_BREAKS + 1)
    pivots = (leave >= 0) & (enter != leave)
    assert (side[pivots] == 1).any()                       # a variable leaves at its upper bound
    if path == "rhs":
        assert _zero_length(t, ns) > 0
        assert not (enter[:ns - 1] == leave[:ns - 1]).any()
    else:
        assert ((enter == leave) & (leave >= 0)).any()     # a bound flip
        if want == OPTIMAL:
            assert t[ns] == np.inf
    # z* is concave (max, RHS; min, cost) or convex in t: the slopes are monotone up to rounding
    rising = (path == "rhs") != bool(maximize)
    d = np.diff(slope)
    tol = 1e-9 * (1.0 + np.abs(slope).max())
    assert (d >= -tol).all() if rising else (d <= tol).all()
    assert np.all(np.diff(t[:ns]) >= 0.0)


@pytest.mark.parametrize("path,reverse", L.TALL)
def test_tall_cases_tie_across_the_seam(path, reverse):
    m, n = L.TALL_SHAPE
    k = n - m
    cs = L.tall(path, reverse)
    r = L.ref(("tall", reverse), path, cs, max_breaks=L.TALL_BREAKS)
    ns, t, slope, enter, leave, side = _path(r)
    assert r["status"] == ITER_LIMIT and ns == L.TALL_BREAKS + 1
    assert t[1] == 1.0 / 64 and t[2] == t[1]               # the tie, and its partner at the same t
    assert _zero_length(t, ns) > 0
    assert (side[(leave >= 0) & (enter != leave)] == 1).any()
    if path == "rhs":
        t0, t1 = L.TIE_ROWS
        # the first POSITION wins: row t0's slack in order, row t1's when the basis is reversed
        assert leave[0] == (k + t1 if reverse else k + t0) and leave[1] == (k + t0 if reverse else k + t1)
    else:
        j0, j1 = L.TIE_COLS
        assert enter[0] == j0 and enter[1] == j1           # the first COLUMN wins
        flips = enter[(enter == leave) & (leave >= 0)]
        assert (flips >= 1024).any() and (enter >= 1024).any()


def test_tall_cases_leave_from_positions_beyond_1024():
    m, n = L.TALL_SHAPE
    for path in L.PATHS:
        seen = False
        for reverse in (False, True):
            cs = L.tall(path, reverse)
            r = L.ref(("tall", reverse), path, cs, max_breaks=L.TALL_BREAKS)
            ns, t, slope, enter, leave, side = _path(r)
            pos = {int(v): p for p, v in enumerate(cs[5])}   # position of a variable of the starting basis
            first = [pos[int(v)] for v in leave if int(v) in pos]
            seen = seen or any(p >= 1024 for p in first)
        assert seen, path


def test_eps_edges_of_the_in_order_tall_rhs_case():
    cs = L.tall("rhs", False)
    k = L.TALL_SHAPE[1] - L.TALL_SHAPE[0]
    firsts = []
    for eps in (0.0, np.nextafter(8.0, 0.0), 8.0):
        r = L.ref(("tall", False), "rhs", cs, eps=eps, max_breaks=L.TALL_BREAKS)
        firsts.append((r["status"], r["nseg"], int(r["leave"][0])))
    assert firsts[0][2] == firsts[1][2] == k + L.TIE_ROWS[0]
    # at eps = 8 the tied pair (delta = -8) is no candidate any more, nor is anything else: the path ends at +inf
    assert firsts[2] == (OPTIMAL, 1, -1)
