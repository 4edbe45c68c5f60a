"""The inputs of tests/tallcases.py on the CPU references alone (no GPU): each must do what its name says — put its
near-tie across (or wholly beyond) row or column 1024 and decide it by eps — or the GPU parity tests of
tests/test_gpu_tall_seams.py would pass without looking at the seams of the HBM-tableau selectors.  Conditions, not
measurements: every case must hold, none is left out.

With max_iter = 1 a result names the one choice made: the basis position that no longer holds its slack is the leaving
row, the variable now there the entering column; a bound flip changes no position and counts in iters."""
import numpy as np
import pytest

from tests import bounded_rules_ref as RR
from tests import tallcases as C
from tests import tolcases as T

DANTZIG, BLAND, DEVEX = RR.RULES
RULES = RR.RULES
ITER_LIMIT = 2
M, N = C.TALL
NO = N - M


def leaving(r, A):
    """The one position that changed, -1 if none did."""
    ch = C.changed(r, A)
    assert len(ch) <= 1
    return ch[0] if ch else -1


def entered(r, A):
    t = leaving(r, A)
    return -1 if t < 0 else int(r["basis"][t])


def sides(name, lo, hi):
    """The stated sides of 1024 for a pair (lo, hi) by the family's name."""
    assert lo < hi
    if name.startswith(("straddle", "upper_twin@straddle")) or name.endswith(("@1024", "@1025")):
        return lo < C.SEAM <= hi
    if "beyond" in name:
        return C.SEAM <= lo
    return True


# ---- the near-tie pairs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.ROW_PAIRS))
def test_row_pairs(name):
    """The first pivot leaves on q at eps = 0 and on p at 1e-12, from the same entering column, for the oracle and for
    bounded_rules_ref.resolve with hi = inf under Dantzig's and the Devex rule, and in its Bland form under Bland's;
    the two ratios differ by at most 4 ulp; p and q lie on the stated sides of 1024."""
    cs = C.case(name)
    p, q = cs.rows
    assert sides(name, p, q) and q < M
    if name == "straddle_rows@m-1":
        assert q == M - 1
    assert 1 <= C.ulps(C.ratio(cs, p), C.ratio(cs, q)) <= 4 and C.ratio(cs, q) < C.ratio(cs, p)
    for eps, row in zip(C.PAIR_EPS, (q, p)):
        assert C.ref_oracle(cs, eps, 1)["trace"] == [(cs.e, row)], (name, eps)
        for rule in (DANTZIG, DEVEX):
            r = C.ref_resolve(cs, eps, 1, rule)
            assert (leaving(r, cs.A), entered(r, cs.A), r["iters"]) == (row, cs.e, [0, 1, 0]), (name, eps, rule)
            assert np.array_equal(r["basis"], C.ref_oracle(cs, eps, 1)["basis"])
        bl = C.bland_form(cs)
        r = C.ref_resolve(bl, eps, 1, BLAND)
        assert (leaving(r, bl.A), entered(r, bl.A), r["iters"]) == (row, 0, [0, 1, 0]), (name, eps)
        bx = C.boxed(cs)     # the box recipe leaves the first pivot alone
        assert leaving(C.ref_resolve(bx, eps, 1), bx.A) == row


def test_late_rows():
    """The near-tie pair (p, q) lies in the first tile and decides nothing: row LATE_WINNER, in the second tile, leaves
    at both eps.  Without that row the pair would decide (q at eps = 0, p at 1e-12): the first tile's scan takes its
    near-tie replay at 1e-12 and must still go on to the second tile."""
    cs = C.case("late_rows")
    p, q = cs.rows
    w = C.LATE_WINNER
    assert p < q < C.SEAM <= w
    assert 1 <= C.ulps(C.ratio(cs, p), C.ratio(cs, q)) <= 4 and C.ratio(cs, q) < C.ratio(cs, p)
    ratios = cs.b / cs.A[:, cs.e]
    assert sorted(np.argsort(ratios)[:3].tolist()) == sorted([w, p, q]) and ratios[w] < 0.75 * ratios[q]
    for eps in C.PAIR_EPS:
        assert C.ref_oracle(cs, eps, 1)["trace"] == [(cs.e, w)]
        for rule in (DANTZIG, DEVEX):
            assert leaving(C.ref_resolve(cs, eps, 1, rule), cs.A) == w
        bl = C.bland_form(cs)
        assert leaving(C.ref_resolve(bl, eps, 1, BLAND), bl.A) == w


@pytest.mark.parametrize("name", list(C.COL_PAIRS))
def test_col_pairs(name):
    """Column e2 enters at eps = 0 and column e at 1e-12 under Dantzig's rule (the oracle and the bounded reference);
    their costs differ by one ulp; the Devex rule takes e2 at both eps (its first arg-max is exact)."""
    cs = C.case(name)
    e, e2 = cs.cols
    assert sides(name, e, e2) and e2 < NO and e == cs.e
    assert C.ulps(cs.c[e], cs.c[e2]) == 1 and cs.c[e2] > cs.c[e]
    for eps, col in zip(C.PAIR_EPS, (e2, e)):
        assert C.ref_oracle(cs, eps, 1)["trace"][0][0] == col, (name, eps)
        assert entered(C.ref_resolve(cs, eps, 1, DANTZIG), cs.A) == col, (name, eps)
        assert entered(C.ref_resolve(C.boxed(cs), eps, 1, DANTZIG), cs.A) == col, (name, eps)
        assert entered(C.ref_resolve(cs, eps, 1, DEVEX), cs.A) == e2, (name, eps)


@pytest.mark.parametrize("name", list(C.DUP_COLS) + list(C.DUP_WIDE))
def test_dup_cols(name):
    """The smaller index of two identical columns enters under every rule at eps 0, 1e-12 and 1e-2 (Bland's in its own
    form, where the smaller index is 0), from the slack basis and, in the cold form, in phase I."""
    cs = C.case(name)
    m, n = cs.A.shape
    e, e2 = cs.cols
    assert e < e2 < n - m and np.array_equal(cs.A[:, e], cs.A[:, e2]) and cs.c[e] == cs.c[e2]
    if name in C.DUP_WIDE:
        assert e2 - e == 4096
    for eps in C.EPS:
        assert C.ref_oracle(cs, eps, 1)["trace"][0][0] == e, (name, eps)
        for rule in RULES:
            form = C.bland_form(cs) if rule == BLAND else cs
            assert entered(C.ref_resolve(form, eps, 1, rule), form.A) == form.e, (name, eps, rule)
            cold = C.cold_form(cs, rule)
            r = C.ref_cold(cold, eps, 1, rule)
            assert r["status"] == ITER_LIMIT and r["iters"] == [1, 0, 0, 0]
            assert [int(v) for v in r["basis"] if v < n] == [cold.e], (name, eps, rule)


@pytest.mark.parametrize("name", list(C.TINY))
def test_tiny_entries(name):
    """The degenerate row q lies past 1024; at eps = 0 the first pivot is on its tiny entry, at 1e-12 on row p."""
    cs = C.case(name)
    p, q = cs.rows
    u = C.TINY[name][0]
    assert q >= C.SEAM and cs.A[q, cs.e] == u and cs.b[q] == 0.0 and u in T.TINY
    for eps, row in zip(C.PAIR_EPS, (q, p)):
        assert C.ref_oracle(cs, eps, 1)["trace"] == [(cs.e, row)], (name, eps)
        assert leaving(C.ref_resolve(cs, eps, 1), cs.A) == row, (name, eps)


# ---- decisions of the bounded kernels alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.UPPER_TWIN))
def test_upper_twin(name):
    """A row leaving at its lower bound against a row leaving at its upper bound: at eps = 0 position q changed and
    at_upper of the leaving slack is 1, at 1e-12 position p changed (under the three rules); one ulp more on U and p
    leaves at both eps.  The two steps differ by less than 1e-13 (U = 1 + s b_p is rounded at 2^-52, the twin's ratio
    finer, so the steps are near but not within 4 ulp)."""
    cs = C.case(name)
    p, q = cs.rows
    assert sides(name, p, q) and abs(cs.nudge) <= 8
    U = cs.hi[NO + q]
    step_q = (cs.b[q] - U) / cs.A[q, cs.e]
    assert cs.A[q, cs.e] < 0 and 0 < C.ratio(cs, p) - step_q < 1e-13
    for rule in RULES:
        form = C.bland_form(cs) if rule == BLAND else cs
        r0, r12 = (C.ref_resolve(form, eps, 1, rule) for eps in C.PAIR_EPS)
        assert leaving(r0, form.A) == q and r0["at_upper"][NO + q] == 1 and r0["iters"] == [0, 1, 0], (name, rule)
        assert leaving(r12, form.A) == p and r12["at_upper"].sum() == 0, (name, rule)
    hi = cs.hi.copy()
    hi[NO + q] = np.nextafter(U, np.inf)
    for eps in C.PAIR_EPS:
        r = RR.resolve(cs.A, cs.b, cs.c, cs.lo, hi, *RR.slack_start(cs.A), True, NO, eps, 1)
        assert leaving(r, cs.A) == p


@pytest.mark.parametrize("theta_eps", C.PAIR_EPS)
def test_flip_edge(theta_eps):
    """The bound flip against the pivot (ue <= theta), theta the chain's first ratio at theta_eps, the winning row past
    1024: under Dantzig's and the Devex rule at eps = theta_eps, "below" and "equal" flip (iters [0, 0, 1], at_upper of
    e set, no position changed) and "above" pivots ([0, 1, 0])."""
    base = C.case(C.FLIP_BASE)
    p, q = base.rows
    assert C.SEAM <= p < q
    for which in C.FLIP_WHICH:
        for form in (C.flip_edge(which, theta_eps), C.flip_boxed(C.flip_edge(which, theta_eps))):
            for rule in (DANTZIG, DEVEX):
                r = C.ref_resolve(form, theta_eps, 1, rule)
                if which == "above":
                    assert r["iters"] == [0, 1, 0] and leaving(r, form.A) == (q if theta_eps == 0.0 else p)
                else:
                    assert r["iters"] == [0, 0, 1] and leaving(r, form.A) == -1 and r["at_upper"][form.e] == 1


def test_flip_edge_bland():
    """Under Bland's rule, in the Bland form (e = 0, the smallest key) with theta the exact minimum ratio: "below" and
    "equal" flip at both eps; "above" pivots on q at eps = 0 and FLIPS at 1e-12, because the entering variable blocks
    when ue <= theta* + eps and key 0 is smaller than every row's."""
    q = C.case(C.FLIP_BASE).rows[1]
    for which in C.FLIP_WHICH:
        form = C.bland_form(C.flip_edge(which, 0.0))
        for eps in C.PAIR_EPS:
            r = C.ref_resolve(form, eps, 1, BLAND)
            if which == "above" and eps == 0.0:
                assert r["iters"] == [0, 1, 0] and leaving(r, form.A) == q
            else:
                assert r["iters"] == [0, 0, 1] and leaving(r, form.A) == -1 and r["at_upper"][0] == 1


# ---- the dual loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.DUAL_KINDS)
@pytest.mark.parametrize("pair", C.DUAL_POSITIONS, ids=lambda v: f"{v[0]},{v[1]}")
def test_dual_rows(kind, pair):
    """One dual pivot: position q changed at eps = 0 and position p at 1e-12; a row violated above leaves complemented
    (at_upper of its slack 1).  The plain dual re-solve agrees on below_below (hi = inf).  Positions: one straddling
    1024 and two beyond it."""
    cs = C.dual_rows(kind, pair)
    p, q = pair
    assert (p < C.SEAM <= q) or C.SEAM <= p
    above = [side == "above" for side in kind.split("_")]
    for form in (cs, C.dual_boxed(cs)):
        for eps, row, up in zip(C.PAIR_EPS, (q, p), (above[1], above[0])):
            r = C.ref_resolve(form, eps, 1)
            assert r["status"] == ITER_LIMIT and r["iters"] == [1, 0, 0], (kind, pair, eps)
            assert leaving(r, form.A) == row and r["at_upper"][NO + row] == int(up), (kind, pair, eps)
    if kind == "below_below":
        for eps, row in zip(C.PAIR_EPS, (q, p)):
            r, d = C.ref_resolve(cs, eps, 1), C.ref_dual(cs, eps, 1)
            assert d["iters"] == (1, 0) and np.array_equal(d["basis"], r["basis"]) and leaving(d, cs.A) == row


@pytest.mark.parametrize("name", list(C.DUAL_COLS))
def test_dual_cols(name):
    """One dual pivot on row DUAL_COL_ROW: column e2 enters at eps = 0 and column e at 1e-12, for the bounded reference
    and the plain dual re-solve; the two quotients differ by at most 4 ulp."""
    cs = C.dual_cols(name)
    e, e2 = cs.cols
    r = C.DUAL_COL_ROW
    assert r >= C.SEAM and e < e2 < NO
    assert (e < C.SEAM <= e2) if name.endswith(("@1024", "@1025")) else (C.SEAM <= e) == ("beyond" in name)
    qe, qe2 = cs.c[e] / cs.A[r, e], cs.c[e2] / cs.A[r, e2]
    assert qe2 < qe and 1 <= C.ulps(qe, qe2) <= 4
    for eps, col in zip(C.PAIR_EPS, (e2, e)):
        for form in (cs, C.dual_boxed(cs)):
            res = C.ref_resolve(form, eps, 1)
            assert res["iters"] == [1, 0, 0] and leaving(res, form.A) == r and entered(res, form.A) == col, (name, eps)
        d = C.ref_dual(cs, eps, 1)
        assert d["iters"] == (1, 0) and np.array_equal(d["basis"], C.ref_resolve(cs, eps, 1)["basis"])


# ---- the cold solve --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.ROW_PAIRS))
def test_cold_forms(name):
    """max_iter = 1: phase I's single pivot enters e and lies on q at eps = 0 and on p at 1e-12, under Dantzig's and the
    Devex rule and, with e at index 0, under Bland's."""
    cs = C.case(name)
    p, q = cs.rows
    for rule in RULES:
        cold = C.cold_form(cs, rule)
        assert np.isinf(cold.hi[cold.e]) and np.isfinite(cold.hi).any()
        for eps, row in zip(C.PAIR_EPS, (q, p)):
            r = C.ref_cold(cold, eps, 1, rule)
            assert r["status"] == ITER_LIMIT and r["iters"] == [1, 0, 0, 0], (name, rule, eps)
            art = np.arange(N, N + M)
            assert np.flatnonzero(r["basis"] != art).tolist() == [row] and r["basis"][row] == cold.e, (name, rule, eps)


# ---- longer runs -----------------------------------------------------------------------------------------------------
def _outcome(r):
    return (np.asarray(r["basis"]).tolist(), list(r["iters"]), np.asarray(r["at_upper"]).tolist())


@pytest.mark.parametrize("name", list(C.ROW_PAIRS) + list(C.COL_PAIRS))
def test_longer_runs_depend_on_eps(name):
    """max_iter = 8: the results at eps = 0 and at 1e-12 differ (basis, iters or at_upper), for the plain and the boxed
    form, so that the run pins more than its first choice."""
    cs = C.case(name)
    for form in (cs, C.boxed(cs)):
        r0, r12 = (C.ref_resolve(form, eps, 8) for eps in C.PAIR_EPS)
        assert sum(r0["iters"]) == sum(r12["iters"]) == 8
        assert _outcome(r0) != _outcome(r12), name
    o0, o12 = (C.ref_oracle(cs, eps, 8) for eps in C.PAIR_EPS)
    assert o0["trace"] != o12["trace"] and len(o0["trace"]) == 8


def test_inputs_without_the_new_arguments_are_unchanged():
    """pair= and cols= absent: the stated seeds still place the pairs the issue's probes found."""
    from oracle import pyoracle as o
    A, b, c, basis = T.near_tie_rows(11, M, N, 1024)
    rows = [o.simplex_tableau(A, b, c, basis, True, NO, eps=e, max_iter=1, trace_cap=1)["trace"][0][1]
            for e in C.PAIR_EPS]
    assert rows == [1055, 31]
