"""CPU-only checks of the dual solution and ranging of a bounded-variable LP at a basis: the test restatement
(tests/ref/bounded_sens_ref.c) against plain numpy formulas at the optima of tests/ref/bounded_ref.c, every finite end
probed from both sides by the bounded re-solve, the x >= 0 case bit for bit against duals_ref.c / ranging_ref.c, the
flags of basic columns, HiGHS duals (the golden cases), hand-made ties / sides / empty ends, the statuses, and the C
ABI's argument checks and fits predicate without a device."""
import functools
import json
import os

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_ref as B
from tests import bounded_resolve_ref as R
from tests import bounded_sens_ref as S
from tests import duals_ref as D
from tests import ranging_ref as RR
from tests.test_ranging_cpu import _lp

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-9
SHAPES = ((4, 12), (8, 20), (16, 48))
INF = np.inf


@functools.lru_cache(maxsize=None)
def _optima():
    """Every optimal bounded_ref solve of boxed_lp(seed, m, n), seeds 0..59 x SHAPES, with the reference's duals and
    ranges at its basis and flags: a list of dicts."""
    out = []
    for m, n in SHAPES:
        for seed in range(60):
            A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n)
            r = B.bounded(A, b, c, lo, hi, mx)
            if r["status"] != B.OPTIMAL:
                continue
            g = S.duals(A, b, c, lo, hi, r["basis"], r["at_upper"])
            q = S.ranging(A, b, c, lo, hi, r["basis"], r["at_upper"], mx)
            out.append(dict(seed=seed, A=A, b=b, c=c, lo=lo, hi=hi, mx=mx, sol=r, duals=g, ranges=q))
    return out


def _numpy_sens(A, b, c, lo, hi, basis, up, maximize, eps=EPS):
    """x, y, d, w and the ranges from np.linalg.inv (close to the reference, not bit-exact)."""
    m, n = A.shape
    nb = np.setdiff1d(np.arange(n), basis)
    v = np.zeros(n)
    v[nb] = np.where(up[nb] != 0, hi[nb], lo[nb])
    Binv = np.linalg.inv(A[:, basis])
    xB = Binv @ (b - A[:, nb] @ v[nb])
    x = v.copy()
    x[basis] = xB
    y = np.linalg.solve(A[:, basis].T, c[basis])
    d = c - A.T @ y
    d[basis] = 0.0
    w = b @ y + d[nb] @ v[nb]
    L, H = lo[basis], hi[basis]
    b_lo, b_hi = np.full(m, -INF), np.full(m, INF)
    for i in range(m):
        los, his = [], []
        for t in range(m):
            beta = Binv[t, i]
            if beta > eps:
                los.append((L[t] - xB[t]) / beta)
                if np.isfinite(H[t]):
                    his.append((H[t] - xB[t]) / beta)
            elif beta < -eps:
                his.append((L[t] - xB[t]) / beta)
                if np.isfinite(H[t]):
                    los.append((H[t] - xB[t]) / beta)
        if los:
            b_lo[i] = b[i] + max(los)
        if his:
            b_hi[i] = b[i] + min(his)
    c_lo, c_hi = np.full(n, -INF), np.full(n, INF)
    sense = {int(j): bool(maximize) != bool(up[j]) for j in nb}
    for j in nb:
        if sense[int(j)]:
            c_hi[j] = c[j] - d[j]
        else:
            c_lo[j] = c[j] - d[j]
    alpha = Binv @ A
    for t, q in enumerate(basis):
        los, his = [], []
        for j in nb:
            a = alpha[t, j]
            if abs(a) > eps:
                (los if (a > eps) == sense[int(j)] else his).append(d[j] / a)
        if los:
            c_lo[q] = c[q] + max(los)
        if his:
            c_hi[q] = c[q] + min(his)
    return x, y, d, w, b_lo, b_hi, c_lo, c_hi


def _close(a, b, scale):
    inf = np.isinf(b)
    assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf])
    assert np.allclose(a[~inf], b[~inf], rtol=1e-9, atol=1e-9 * scale)


def test_the_cases_cover_upper_bounds_and_flagged_basic_columns():
    cases = _optima()
    at_upper = flagged_basic = 0
    for k in cases:
        basis, up = k["sol"]["basis"], k["sol"]["at_upper"]
        nb = np.setdiff1d(np.arange(len(up)), basis)
        at_upper += int(up[nb].sum())
        flagged_basic += int(up[basis].sum())
    assert len(cases) >= 170 and at_upper >= 100 and flagged_basic >= 5, (len(cases), at_upper, flagged_basic)


@pytest.mark.parametrize("shape", SHAPES)
def test_matches_numpy_at_the_bounded_optimum(shape):
    cases = [k for k in _optima() if k["A"].shape == shape]
    assert cases
    for k in cases:
        A, b, c, lo, hi, mx = (k[key] for key in ("A", "b", "c", "lo", "hi", "mx"))
        sol, g, q = k["sol"], k["duals"], k["ranges"]
        basis, up = sol["basis"], sol["at_upper"]
        n = A.shape[1]
        nb = np.setdiff1d(np.arange(n), basis)
        assert g["status"] == S.OPTIMAL and q["status"] == S.OPTIMAL
        x, y, d, w, b_lo, b_hi, c_lo, c_hi = _numpy_sens(A, b, c, lo, hi, basis, up, mx)
        scale = 1 + np.abs(b).max() + np.abs(c).max()
        _close(g["x"], x, scale)
        _close(g["y"], y, scale)
        _close(g["d"], d, scale)
        assert abs(g["w"] - w) <= 1e-9 * scale * (1 + abs(w))
        for key, want in (("b_lo", b_lo), ("b_hi", b_hi), ("c_lo", c_lo), ("c_hi", c_hi)):
            _close(q[key], want, scale)
        # against the solver: the objective, the point, and the sign of every non-basic reduced cost at EPS
        assert abs(g["w"] - sol["obj"]) <= 1e-7 * (1 + abs(sol["obj"])), k["seed"]
        assert np.allclose(g["x"], sol["x"], rtol=0, atol=1e-7 * (1 + np.abs(sol["x"]).max())), k["seed"]
        assert np.array_equal(S.bits(g["d"][basis]), S.bits(np.zeros(len(basis))))
        sgn = 1.0 if mx else -1.0
        assert (sgn * g["d"][nb][up[nb] == 0] <= EPS).all(), k["seed"]
        assert (sgn * g["d"][nb][up[nb] == 1] >= -EPS).all(), k["seed"]
        # the current value lies in its own range
        assert (q["b_lo"] <= b + 1e-9).all() and (b <= q["b_hi"] + 1e-9).all(), k["seed"]
        assert (q["c_lo"] <= c + 1e-9).all() and (c <= q["c_hi"] + 1e-9).all(), k["seed"]
        # indices: the leaving column is basic, the entering one non-basic, -1 exactly at infinite ends
        for lo_, hi_, idx in ((q["b_lo"], q["b_hi"], q["b_leave"]), (q["b_lo"], q["b_hi"], q["b_side"]),
                              (q["c_lo"], q["c_hi"], q["c_enter"])):
            assert np.array_equal(idx[:, 0] < 0, np.isinf(lo_)) and np.array_equal(idx[:, 1] < 0, np.isinf(hi_))
        assert set(q["b_leave"][q["b_leave"] >= 0].tolist()) <= set(basis.tolist())
        assert not set(q["c_enter"][q["c_enter"] >= 0].tolist()) & set(basis.tolist())
        assert set(np.unique(q["b_side"]).tolist()) <= {-1, 0, 1}
        side1 = q["b_leave"][q["b_side"] == 1]
        assert np.isfinite(hi[side1]).all()   # a variable leaves at its upper bound only if it has one


def test_each_finite_end_holds_inside_and_fails_outside():
    """Per LP three rows and four columns: b_i (c_j) moved 0.9 of the way to a finite end keeps the basis and flags
    optimal without a pivot or flip in the bounded re-solve; moved 1.1 of the way it does not."""
    counts = dict(b_in=0, b_out=0, c_in=0, c_out=0)
    for k in _optima():
        A, b, c, lo, hi, mx = (k[key] for key in ("A", "b", "c", "lo", "hi", "mx"))
        sol, q = k["sol"], k["ranges"]
        m, n = A.shape
        rng = np.random.default_rng(k["seed"])
        rows = rng.choice(m, size=3, replace=False)
        cols = rng.choice(n, size=4, replace=False)

        def stays(b2, c2):
            r = R.resolve(A, b2, c2, lo, hi, sol["basis"], sol["at_upper"], mx)
            return r["status"] == R.OPTIMAL and r["iters"] == [0, 0, 0]

        for what, picks, cur, ends in (("b", rows, b, (q["b_lo"], q["b_hi"])), ("c", cols, c, (q["c_lo"], q["c_hi"]))):
            for i in picks:
                for end in ends:
                    if not np.isfinite(end[i]) or abs(end[i] - cur[i]) < 1e-6:
                        continue
                    for f, want in ((0.9, True), (1.1, False)):
                        moved = cur.copy()
                        moved[i] = cur[i] + f * (end[i] - cur[i])
                        got = stays(moved, c) if what == "b" else stays(b, moved)
                        assert got == want, (A.shape, k["seed"], what, int(i), f)
                        counts[what + ("_in" if want else "_out")] += 1
    assert min(counts.values()) > 0, counts


@pytest.mark.parametrize("seed", range(20))
def test_without_bounds_it_is_the_unbounded_references_bits(seed):
    A, b, c, basis, mx = _lp(seed)
    n = A.shape[1]
    lo, hi, up = np.zeros(n), np.full(n, INF), np.zeros(n, np.int32)
    g, g0 = S.duals(A, b, c, lo, hi, basis, up), D.duals(A, b, c, basis)
    assert g["status"] == g0["status"]
    S.same_bits(g, g0, ("y", "d", "w"))
    q, q0 = S.ranging(A, b, c, lo, hi, basis, up, mx), RR.ranging(A, b, c, basis, mx)
    assert q["status"] == q0["status"]
    S.same_bits(q, q0, ("b_lo", "b_hi", "b_leave", "c_lo", "c_hi", "c_enter"))
    assert set(np.unique(q["b_side"]).tolist()) <= {-1, 0}


def test_flags_of_basic_columns_are_not_read():
    seen = 0
    for k in _optima()[:60]:
        A, b, c, lo, hi, mx = (k[key] for key in ("A", "b", "c", "lo", "hi", "mx"))
        basis, up = k["sol"]["basis"], k["sol"]["at_upper"]
        boxed = [int(j) for j in basis if np.isfinite(hi[j])]
        if not boxed:
            continue
        up2 = up.copy()
        up2[boxed] ^= 1
        g = S.duals(A, b, c, lo, hi, basis, up2)
        q = S.ranging(A, b, c, lo, hi, basis, up2, mx)
        assert g["status"] == S.OPTIMAL and q["status"] == S.OPTIMAL
        S.same_bits(g, k["duals"], S.DUALS_KEYS)
        S.same_bits(q, k["ranges"], S.RANGING_KEYS)
        seen += 1
    assert seen >= 10


def test_golden_highs_duals():
    cases = json.load(open(os.path.join(HERE, "golden", "bounded_sens_cases.json")))
    assert len(cases) >= 12
    upper = fixed = 0
    senses = set()
    for g in cases:
        assert sorted(g) == ["args", "d_nonbasic", "obj", "y"]
        A, b, c, lo, hi, mx = B.boxed_lp(*g["args"])
        senses.add(bool(mx))
        sol = B.bounded(A, b, c, lo, hi, mx)
        assert sol["status"] == B.OPTIMAL
        basis, up = sol["basis"], sol["at_upper"]
        nb = np.setdiff1d(np.arange(A.shape[1]), basis)
        upper += int(up[nb].sum() > 0)
        fixed += int((lo == hi).any())
        r = S.duals(A, b, c, lo, hi, basis, up)
        assert r["status"] == S.OPTIMAL
        assert abs(r["w"] - g["obj"]) <= 1e-7 * (1 + abs(g["obj"])), g["args"]
        y = np.array(g["y"])
        assert (np.abs(r["y"] - y) <= 1e-7 * (1 + np.abs(y))).all(), g["args"]
        assert [j for j, _ in g["d_nonbasic"]] == nb.tolist(), g["args"]   # the same (unique) basis
        d = np.array([v for _, v in g["d_nonbasic"]])
        assert (np.abs(r["d"][nb] - d) <= 1e-7 * (1 + np.abs(d))).all(), g["args"]
    assert senses == {True, False}
    assert upper >= 1 and fixed >= 1


# max x0 + x1 s.t. x0 + s0 = 1, x1 + s1 = 1, x0 + x1 + s2 = b2 at basis (x0, x1, s2): x0 = x1 = 1, s2 = b2 - 2.
# Column 0 of B^-1 is (1, 0, -1): raising b0 raises x0 and lowers s2.
A35 = np.array([[1.0, 0, 1, 0, 0], [0, 1.0, 0, 1, 0], [1.0, 1, 0, 0, 1]])
C35 = np.array([1.0, 1.0, 0, 0, 0])
BASIS35 = np.array([0, 1, 4], np.int32)
NOFLAG5 = np.zeros(5, np.int32)


def test_ties_take_the_first_position_and_report_its_side():
    lo, hi = np.zeros(5), np.array([2.0, INF, INF, INF, INF])
    # b2 = 3: s2 = 1.  Upper end of b0: x0 reaches hi = 2 at +1 (position 0, side 1), s2 reaches 0 at +1 (position 2)
    q = S.ranging(A35, np.array([1.0, 1.0, 3.0]), C35, lo, hi, BASIS35, NOFLAG5, True)
    assert q["status"] == S.OPTIMAL
    assert q["b_hi"][0] == 2.0 and q["b_leave"][0, 1] == 0 and q["b_side"][0, 1] == 1
    assert q["b_lo"][0] == 0.0 and q["b_leave"][0, 0] == 0 and q["b_side"][0, 0] == 0
    # the same tie with the positions swapped: s2 first
    basis = np.array([4, 1, 0], np.int32)
    q = S.ranging(A35, np.array([1.0, 1.0, 3.0]), C35, lo, hi, basis, NOFLAG5, True)
    assert q["b_hi"][0] == 2.0 and q["b_leave"][0, 1] == 4 and q["b_side"][0, 1] == 0
    # costs: two non-basic columns with equal ratios (column 2 and a copy of it at column 5): the first wins
    A6 = np.hstack([A35, A35[:, 2:3]])
    q = S.ranging(A6, np.array([1.0, 1.0, 3.0]), np.append(C35, 0.0), np.zeros(6), np.full(6, INF), BASIS35,
                  np.zeros(6, np.int32), True)
    assert q["c_lo"][0] == 0.0 and q["c_enter"][0, 0] == 2
    assert q["c_hi"][0] == INF and q["c_enter"][0, 1] == -1


def test_a_row_bounded_from_an_upper_and_from_a_lower_side():
    # b2 = 2.25: s2 = 0.25 with hi = 1; x0 with hi = 1.5
    lo, hi = np.zeros(5), np.array([1.5, INF, INF, INF, 1.0])
    b = np.array([1.0, 1.0, 2.25])
    q = S.ranging(A35, b, C35, lo, hi, BASIS35, NOFLAG5, True)
    assert q["status"] == S.OPTIMAL
    # upper end of b0: x0 -> 1.5 at +0.5, s2 -> 0 at +0.25: s2 leaves at its lower bound
    assert q["b_hi"][0] == 1.25 and q["b_leave"][0, 1] == 4 and q["b_side"][0, 1] == 0
    # lower end of b0: x0 -> 0 at -1, s2 -> 1 at -0.75: s2 leaves at its upper bound
    assert q["b_lo"][0] == 0.25 and q["b_leave"][0, 0] == 4 and q["b_side"][0, 0] == 1
    # row 2 moves s2 alone: [2.25 - 0.25, 2.25 + 0.75], leaving at its lower and at its upper bound
    assert q["b_lo"][2] == 2.0 and q["b_hi"][2] == 3.0
    assert q["b_leave"][2].tolist() == [4, 4] and q["b_side"][2].tolist() == [0, 1]
    g = S.duals(A35, b, C35, lo, hi, BASIS35, NOFLAG5)
    assert g["x"].tolist() == [1.0, 1.0, 0.0, 0.0, 0.25] and g["w"] == 2.0
    # s0 held at an upper bound of 0.5: x0 = 0.5, and s0's cost is ranged with the opposite sense
    hi2 = np.array([1.5, INF, 0.5, INF, 1.0])
    up = np.array([0, 0, 1, 0, 0], np.int32)
    g = S.duals(A35, b, C35, lo, hi2, BASIS35, up)
    assert g["x"].tolist() == [0.5, 1.0, 0.5, 0.0, 0.75] and g["d"][2] == -1.0 and g["w"] == 1.5
    q = S.ranging(A35, b, C35, lo, hi2, BASIS35, up, True)
    assert q["c_lo"][2] == 1.0 and q["c_hi"][2] == INF and q["c_enter"][2].tolist() == [2, -1]
    assert q["c_lo"][3] == -INF and q["c_hi"][3] == 1.0 and q["c_enter"][3].tolist() == [-1, 3]


def test_a_zero_lower_bound_keeps_the_unbounded_signed_zero():
    """The L_t == 0 case of test_ranging_cpu.test_ties_take_the_first_index: -xB / beta, not (0 - xB) / beta."""
    A0 = np.array([[1.0, 0, 1, 0], [0, -1.0, 0, 1]])
    b0, c0 = np.array([0.0, 0.0]), np.array([1.0, 1.0, 0, 0])
    basis = np.array([0, 1], np.int32)
    q = S.ranging(A0, b0, c0, np.zeros(4), np.full(4, INF), basis, np.zeros(4, np.int32), True)
    q0 = RR.ranging(A0, b0, c0, basis, True)
    assert q["b_lo"][0] == 0.0 and not np.signbit(q["b_lo"][0])
    assert q["b_leave"][0, 0] == 0 and q["b_side"][0, 0] == 0
    S.same_bits(q, q0, ("b_lo", "b_hi", "b_leave", "c_lo", "c_hi", "c_enter"))


def test_empty_sides():
    """At the slack basis nothing bounds a row from above: +inf, variable -1, side -1."""
    basis = np.array([2, 3, 4], np.int32)
    q = S.ranging(A35, np.array([1.0, 1.0, 3.0]), C35, np.zeros(5), np.full(5, INF), basis, NOFLAG5, True)
    assert q["status"] == S.OPTIMAL
    assert np.isposinf(q["b_hi"]).all() and (q["b_leave"][:, 1] == -1).all() and (q["b_side"][:, 1] == -1).all()
    assert q["b_lo"].tolist() == [0.0, 0.0, 0.0] and q["b_leave"][:, 0].tolist() == [2, 3, 4]
    assert (q["b_side"][:, 0] == 0).all()
    # with every slack boxed the upper side is bounded too, by the slack's own upper bound
    hi = np.array([INF, INF, 4.0, 4.0, 4.0])
    q = S.ranging(A35, np.array([1.0, 1.0, 3.0]), C35, np.zeros(5), hi, basis, NOFLAG5, True)
    assert q["b_hi"].tolist() == [4.0, 4.0, 4.0] and (q["b_side"][:, 1] == 1).all()


def _all_nan(g, q):
    assert all(np.isnan(np.asarray(g[k])).all() for k in S.DUALS_KEYS)
    assert all(np.isnan(q[k]).all() for k in ("b_lo", "b_hi", "c_lo", "c_hi"))
    assert all((q[k] == -1).all() for k in ("b_leave", "b_side", "c_enter"))


def test_statuses():
    k = _optima()[0]
    A, b, c, lo, hi, mx = (k[key] for key in ("A", "b", "c", "lo", "hi", "mx"))
    basis, up = k["sol"]["basis"], k["sol"]["at_upper"]
    n = A.shape[1]

    def both(lo=lo, hi=hi, basis=basis, up=up, eps=EPS):
        g = S.duals(A, b, c, lo, hi, basis, up)
        q = S.ranging(A, b, c, lo, hi, basis, up, mx, eps)
        return g, q

    rep = basis.copy()
    rep[1] = rep[0]
    g, q = both(basis=rep)
    assert g["status"] == S.SINGULAR and q["status"] == S.SINGULAR
    _all_nan(g, q)
    j = int(np.flatnonzero(np.isfinite(hi))[0]) if np.isfinite(hi).any() else 0
    crossed = hi.copy()
    crossed[j] = lo[j] - 0.5
    g, q = both(hi=crossed)
    assert g["status"] == S.INFEASIBLE and q["status"] == S.INFEASIBLE
    _all_nan(g, q)
    free = int(np.flatnonzero(np.isinf(hi))[0])
    refusals = []
    for bad in (np.nan, INF, -INF):
        v = lo.copy()
        v[0] = bad
        refusals.append(dict(lo=v))
    v = hi.copy()
    v[0] = np.nan
    refusals.append(dict(hi=v))
    for flag, at in ((2, 0), (-1, 0), (1, free)):
        v = np.zeros(n, np.int32)
        v[at] = flag
        refusals.append(dict(up=v))
    for idx in (-1, n):
        v = basis.copy()
        v[1] = idx
        refusals.append(dict(basis=v))
    for kw in refusals:
        g, q = both(**kw)
        assert g["status"] == S.BAD_ARG and q["status"] == S.BAD_ARG, kw
        _all_nan(g, q)
    for eps in (-1e-12, float("nan")):
        q = S.ranging(A, b, c, lo, hi, basis, up, mx, eps)
        assert q["status"] == S.BAD_ARG and np.isnan(q["b_lo"]).all()
    assert S.ranging(A, b, c, lo, hi, basis, up, mx, 0.0)["status"] == S.OPTIMAL


def test_abi_rejects_a_null_context():
    lib = capi.load()
    m, n, batch = 2, 4, 2
    A = np.zeros(batch * m * n)
    b, c = np.ones(batch * m), np.ones(batch * n)
    lo, hi = np.zeros(batch * n), np.ones(batch * n)
    basis, up = np.zeros(batch * m, np.int32), np.zeros(batch * n, np.int32)
    x, y, d, w = np.zeros(batch * n), np.zeros(batch * m), np.zeros(batch * n), np.zeros(batch)
    rhs, cost = np.zeros(batch * 2 * m), np.zeros(batch * 2 * n)
    rv, rs, cv = (np.zeros(batch * 2 * k, np.int32) for k in (m, m, n))
    st = np.zeros(batch, np.int32)
    dp, ip = capi._d, capi._i
    assert lib.lp_basis_bounded_duals(None, dp(A), m, n, dp(b), dp(c), dp(lo), dp(hi), ip(basis), ip(up), dp(x), dp(y),
                                      dp(d), dp(w)) == capi.BAD_ARG
    assert lib.lp_basis_bounded_duals_batched(None, batch, dp(A), m, n, dp(b), dp(c), dp(lo), dp(hi), ip(basis), ip(up),
                                              dp(x), dp(y), dp(d), dp(w), ip(st)) == capi.BAD_ARG
    assert lib.lp_basis_bounded_ranging(None, dp(A), m, n, dp(b), dp(c), dp(lo), dp(hi), ip(basis), ip(up), 1, EPS,
                                        dp(rhs), ip(rv), ip(rs), dp(cost), ip(cv)) == capi.BAD_ARG
    assert lib.lp_basis_bounded_ranging_batched(None, batch, dp(A), m, n, dp(b), dp(c), dp(lo), dp(hi), ip(basis),
                                                ip(up), 1, EPS, dp(rhs), ip(rv), ip(rs), dp(cost), ip(cv),
                                                ip(st)) == capi.BAD_ARG


def _carve_bytes(m, n):
    """The analysis kernel's LDS carve restated (basis_bounded.hip): lp_basis_ranging's plus v (n) and L, H (2m)."""
    pitch = (m + 1) | 1
    scratch = max(256 * 9, 2 * m + 1)
    return 8 * (2 + m * pitch + scratch + 3 * m + 2 * n) + 4 * (4 * m + n)


def test_fits_predicate():
    lib = capi.load()
    for m, n in ((16, 40), (32, 96), (64, 192)):
        assert lib.lp_basis_bounded_fits(m, n) == 1
    for m, n in ((160, 320), (0, 4), (8, 4)):
        assert lib.lp_basis_bounded_fits(m, n) == 0
    # at n = m the analysis kernel's carve is the binding one: 130 x 130 is the last that fits 160 KiB
    assert _carve_bytes(130, 130) <= 160 * 1024 < _carve_bytes(131, 131)
    assert lib.lp_simplex_bounded_fits(131, 131) == 1
    assert lib.lp_basis_bounded_fits(130, 130) == 1 and lib.lp_basis_bounded_fits(131, 131) == 0
    for m in range(1, 140):
        for n in (m, 2 * m, 3 * m):
            want = lib.lp_simplex_bounded_fits(m, n) == 1 and _carve_bytes(m, n) <= 160 * 1024
            assert lib.lp_basis_bounded_fits(m, n) == int(want), (m, n)


# B = diag(-1, 1), b = (-0.0, 0.0): xB_0 = -0.0 / -1 = +0.0 and beta = -1 for row 0's upper end
A_SZ = np.array([[-1.0, 0, 1, 0], [0, 1.0, 0, 1]])
B_SZ = np.array([-0.0, 0.0])
C_SZ = np.array([1.0, 1.0, 0, 0])
BASIS_SZ = np.array([0, 1], np.int32)


def test_the_zero_lower_bound_branch_decides_a_sign():
    """An input where -xB / beta and (0.0 - xB) / beta differ in the reported bits: xB = +0.0, beta = -1, b_i = -0.0.
    -xB / beta = -0.0 / -1 = +0.0 and b_i + 0.0 = +0.0, whereas (0.0 - 0.0) / -1 = -0.0 and b_i + -0.0 = -0.0."""
    lo, hi, up = np.zeros(4), np.full(4, INF), np.zeros(4, np.int32)
    g = S.duals(A_SZ, B_SZ, C_SZ, lo, hi, BASIS_SZ, up)
    assert g["x"][0] == 0.0 and not np.signbit(g["x"][0])
    q = S.ranging(A_SZ, B_SZ, C_SZ, lo, hi, BASIS_SZ, up, True)
    assert q["b_hi"][0] == 0.0 and not np.signbit(q["b_hi"][0])
    assert q["b_leave"][0, 1] == 0 and q["b_side"][0, 1] == 0
    S.same_bits(q, RR.ranging(A_SZ, B_SZ, C_SZ, BASIS_SZ, True), ("b_lo", "b_hi", "b_leave", "c_lo", "c_hi", "c_enter"))
    # with a lower bound that is not 0.0 the numerator is L - xB: the same end, the other way round
    lo2 = np.array([-1.0, 0, 0, 0])
    q = S.ranging(A_SZ, B_SZ, C_SZ, lo2, hi, BASIS_SZ, up, True)
    assert q["b_hi"][0] == 1.0 and q["b_side"][0, 1] == 0   # (-1 - 0) / -1 = 1, b_i + 1


def test_a_flag_under_minus_infinity_is_a_crossed_bound():
    """hi_j = -inf is not 'no upper bound': a flag there is accepted by the checks and the LP is INFEASIBLE."""
    k = _optima()[0]
    A, b, c, lo, mx = (k[key] for key in ("A", "b", "c", "lo", "mx"))
    hi, up = k["hi"].copy(), k["sol"]["at_upper"].copy()
    hi[0], up[0] = -INF, 1
    g = S.duals(A, b, c, lo, hi, k["sol"]["basis"], up)
    q = S.ranging(A, b, c, lo, hi, k["sol"]["basis"], up, mx)
    assert g["status"] == S.INFEASIBLE and q["status"] == S.INFEASIBLE
    _all_nan(g, q)


def test_the_reference_refuses_null_pointers():
    k = _optima()[0]
    A, b, c, lo, hi = (np.ascontiguousarray(k[key], dtype=np.float64) for key in ("A", "b", "c", "lo", "hi"))
    m, n = A.shape
    Af = np.ascontiguousarray(A.T).reshape(-1)
    basis = np.ascontiguousarray(k["sol"]["basis"], dtype=np.int32)
    up = np.ascontiguousarray(k["sol"]["at_upper"], dtype=np.int32)
    x, y, d, w = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(1)
    rhs, cost = np.zeros(2 * m), np.zeros(2 * n)
    rv, rs, cv = np.zeros(2 * m, np.int32), np.zeros(2 * m, np.int32), np.zeros(2 * n, np.int32)
    L, dp, ip = S.lib(), S._d, S._i
    duals = [dp(Af), m, n, dp(b), dp(c), dp(lo), dp(hi), ip(basis), ip(up), dp(x), dp(y), dp(d), dp(w)]
    ranging = [dp(Af), m, n, dp(b), dp(c), dp(lo), dp(hi), ip(basis), ip(up), 1, EPS, dp(rhs), ip(rv), ip(rs), dp(cost),
               ip(cv)]
    assert L.ref_bounded_duals(*duals) == S.OPTIMAL and L.ref_bounded_ranging(*ranging) == S.OPTIMAL
    for fn, args, pointers in ((L.ref_bounded_duals, duals, (0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)),
                               (L.ref_bounded_ranging, ranging, (0, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15))):
        for at in pointers:
            bad = list(args)
            bad[at] = None
            assert fn(*bad) == S.BAD_ARG, (fn.__name__, at)
