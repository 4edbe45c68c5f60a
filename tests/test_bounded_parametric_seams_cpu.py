"""What the cases of tests/bounded_parametric_seam_cases.py promise, asserted on the reference alone (no GPU), so that
tests/test_gpu_bounded_parametric_seams.py cannot quietly lose its coverage: the seam relation of the pinned indices
(computed from SCAN, TILE, GATHER and CHUNK), the first breakpoint at t = 1/64 with the intended enter, leave and side
at eps = 0 and eps = 1e-12 (different answers wherever the family is a near-tie), the flips that flip and the pivots that
pivot, the flagged starts, what max_breaks = 0 leaves, the statuses over the whole grid, and that every seam of the
entering chain and of the ratio test has a near-tie pair across it and one wholly beyond it on each path."""
import numpy as np
import pytest

from tests import bounded_parametric_large_cases as L
from tests import bounded_parametric_seam_cases as S

OPTIMAL, UNBOUNDED, ITER_LIMIT, INFEASIBLE = L.OPTIMAL, L.UNBOUNDED, L.ITER_LIMIT, L.INFEASIBLE


@pytest.mark.parametrize("name", S.NAMES)
def test_pinned_indices_lie_where_the_name_says(name):
    cs = S.CASES[name]
    m, n = S.SHAPES[cs.shape]
    p, q = cs.pair
    assert cs.rel or cs.space == "tau", name
    for rel in cs.rel:
        assert S.RELATIONS[rel](p, q), (name, rel)
    limit = (n - m) if (cs.space == "col" or (cs.space == "tau" and cs.path == "cost")) else m
    assert 0 <= p < limit and (q is None or p < q < limit)
    assert cs.near == (cs.first[0.0] != cs.first[1e-12])


@pytest.mark.parametrize("name", S.NAMES)
def test_first_breakpoint_is_the_intended_one(name):
    cs = S.CASES[name]
    case = cs.make()
    A, b, c, lo, hi, basis, up, direction, _ = case
    m, n = A.shape
    assert (m, n) == S.SHAPES[cs.shape] and not lo.any()
    assert np.array_equal(np.sort(basis), np.arange(n - m, n)) and (basis[0] > basis[1]) == cs.reverse
    got = {}
    for eps in (0.0, 1e-12):
        r = S.ref(name, case, eps, 1)
        assert r["nseg"] >= 1 and r["t"][0] == 0.0 and r["t"][1] == S.TAU, (name, eps)
        got[eps] = (int(r["enter"][0]), int(r["leave"][0]), int(r["side"][0]))
        assert got[eps] == cs.first[eps], (name, eps, got[eps])
        if cs.flip is not None:
            assert (got[eps][0] == got[eps][1]) == cs.flip[eps], (name, eps)
        if cs.path == "rhs" and got[eps][0] >= 0:
            assert r["status"] in (ITER_LIMIT, INFEASIBLE, OPTIMAL) and got[eps][0] != got[eps][1]
    assert (got[0.0] != got[1e-12]) == cs.near, name
    # the pinned POSITIONS are where the catalogue says, whichever rows the basis order puts there
    p, q = cs.pair
    if cs.space == "tau" and cs.path == "rhs":
        assert basis[p] == got[0.0][1]
    elif cs.space == "pos":
        for eps, pos in ((0.0, q if cs.near else p), (1e-12, p)):
            if got[eps][0] != got[eps][1]:
                assert basis[pos] == got[eps][1], (name, eps)
    # the largest eps of the grid decides as 1e-12 does (the pinned values differ by an ulp, or by 2^-41)
    r = S.ref(name, case, 1e-2, 1)
    assert (int(r["enter"][0]), int(r["leave"][0]), int(r["side"][0])) == cs.first[1e-12], name
    if cs.flagged:
        k = n - m
        flagged = np.flatnonzero(up[:k])
        assert r["obj"][0] != 0.0 and len(flagged) >= 300
        assert set(flagged // S.CHUNK) == set(range((k + S.CHUNK - 1) // S.CHUNK))
        for j in (S.CHUNK - 1, S.CHUNK, S.TILE - 1, S.TILE, 2 * S.TILE - 1, 2 * S.TILE, k - 1):
            assert j >= k or up[j] == 1, j
        columns = cs.space == "col" or (cs.space == "tau" and cs.path == "cost")
        pinned = [j for j in cs.pair if j is not None] if columns else []
        assert not up[pinned].any() and not up[r["enter"][0]]
        assert np.all(c[flagged] <= 0.0) and np.all(c[:k][up[:k] == 0] >= 0.0)
    else:
        assert r["obj"][0] == 0.0


def test_slack_flagged_case_has_up_set_at_the_leaving_variable():
    (name,) = [nm for nm in S.NAMES if "slackup" in nm]
    cs = S.CASES[name]
    case = cs.make()
    r = S.ref(name, case, 0.0, 1)
    leave = int(r["leave"][0])
    assert case[6][leave] == 1 and r["side"][0] == 0 and cs.flagged   # up = 1, blocked above: side = up ^ 1


def test_flip_families_rewrite_rows_past_the_seams():
    for name in S.NAMES:
        cs = S.CASES[name]
        if cs.flip is None:
            continue
        case = cs.make()
        m = case[0].shape[0]
        e = cs.first[0.0][0]
        col = case[0][:, e] if not cs.reverse else case[0][::-1, e]
        for pos in (965, 1025, m - 1):
            assert col[pos] != 0.0, (name, pos)
        assert np.count_nonzero(col[S.SCAN:]) > 50
    kinds = {nm.split("@")[0] for nm in S.NAMES if S.CASES[nm].flip is not None}
    assert kinds == {"cost-flip_below", "cost-flip_equal", "cost-flip_above"}


_statuses = {}


def _walk(name, epss=S.EPS):
    """The grid of one case at some eps: what max_breaks = 0 leaves, and the statuses reached."""
    if (name, epss) in _statuses:
        return _statuses[name, epss]
    cs = S.CASES[name]
    case = cs.make()
    seen = set()
    for eps, mb in ((eps, mb) for eps in epss for mb in S.BREAKS):
        r = S.ref(name, case, eps, mb)
        seen.add(int(r["status"]))
        ns = r["nseg"]
        assert 1 <= ns <= mb + 1, (name, eps, mb)
        if mb == 0:   # the blocking row or column leaves no trace: the basis and the flags are the start's
            assert np.array_equal(r["basis"], case[5]) and np.array_equal(r["at_upper"], case[6])
            if cs.path == "rhs":
                assert r["leave"][0] >= 0 and r["side"][0] in (0, 1) and r["enter"][0] == -1
                assert r["status"] == (INFEASIBLE if "no_entering" in name else ITER_LIMIT)
            else:
                assert r["enter"][0] >= 0 and r["leave"][0] == -1 and r["side"][0] == -1
                assert r["status"] == ITER_LIMIT
    if name in S.EDGE_CASE.values() and epss == S.EPS:
        for t_max in S.EDGE_TMAX:
            r = S.ref(name, case, 0.0, S.EDGE_BREAKS, t_max=t_max)
            seen.add(int(r["status"]))
            if t_max <= S.TAU:   # t* >= t_max: the path ends at t_max
                assert (r["status"], r["nseg"], r["t"][1]) == (OPTIMAL, 1, t_max)
                assert r["enter"][0] == r["leave"][0] == r["side"][0] == -1
            else:
                assert r["nseg"] > 1 and r["t"][1] == S.TAU
        under, at = (S.ref(name, case, eps, S.EDGE_BREAKS) for eps in S.EDGE_EPS[cs.path])
        # at eps = |delta_r| or |g_e| the pinned candidate is none any more; just below it still is one
        assert under["t"][1] == S.TAU and at["t"][1] != S.TAU
        seen.update((int(under["status"]), int(at["status"])))
    _statuses[name, epss] = seen
    return seen


@pytest.mark.parametrize("name,epss", S.GRID_PARAMS, ids=S.GRID_IDS)
def test_grid_of_every_case(name, epss):
    assert _walk(name, epss) <= {OPTIMAL, UNBOUNDED, ITER_LIMIT, INFEASIBLE}


def test_statuses_reached_over_the_grid():
    by_path = {path: set() for path in L.PATHS}
    assert {nm for nm, _ in S.GRID_PARAMS} == set(S.NAMES)
    assert sorted(eps for nm, epss in S.GRID_PARAMS for eps in epss) == sorted(S.EPS * len(S.NAMES))
    assert not set(S.EDGE_CASE.values()) & set(S.CRASHED)
    for name, epss in S.GRID_PARAMS:
        by_path[S.CASES[name].path] |= _walk(name, epss)
    assert {OPTIMAL, ITER_LIMIT, INFEASIBLE} <= by_path["rhs"]
    assert {OPTIMAL, ITER_LIMIT} <= by_path["cost"]


def test_every_seam_has_a_pair_across_it_and_one_beyond_it():
    for path, space in (("rhs", "col"), ("cost", "pos")):
        pairs = [c.pair for c in S.CASES.values() if c.path == path and c.space == space and c.near]
        for seam in (S.SCAN, 2 * S.SCAN, S.TILE, 2 * S.TILE):
            assert any(p < seam <= q for p, q in pairs), (path, seam)
            assert any(seam <= p for p, q in pairs), (path, seam)
        assert any(q == p + S.SCAN for p, q in pairs) and any(q == p + 2 * S.SCAN for p, q in pairs)
    for path in L.PATHS:
        ties = [c for c in S.CASES.values() if c.path == path and c.space == "tau" and c.pair[1] is not None]
        assert any(S.wave_of(c.pair[0]) == 15 and S.wave_of(c.pair[1]) != 15 for c in ties), path
        assert any(S.wave_of(c.pair[0]) != 15 and c.pair[1] >= S.GATHER for c in ties), path
        assert any(S.wave_of(c.pair[0]) == 15 and S.wave_of(c.pair[1]) == 15 for c in ties), path
        assert any(c.path == path and c.space == "tau" and c.pair[1] is None for c in S.CASES.values()), path
    for path in L.PATHS:
        assert {c.shape for c in S.CASES.values() if c.path == path and c.flagged} >= {"TALL", "WIDE"}
        assert any(c.reverse for c in S.CASES.values() if c.path == path)
    assert {c.name.split("@")[0].split("-", 1)[1] for c in S.CASES.values() if c.reverse} == {
        "same_thread", "beyond", "tau_tie", "flip_equal"}
