"""CPU-only checks of the parametric right-hand-side path: the test restatement (tests/ref/parametric_ref.c) against
HiGHS objectives along every path (the golden cases), the path's own algebra (values on each segment's line,
continuity at every breakpoint, concave for max and convex for min, the first slope as y.d), bit-exact agreement
with the RHS ranging of tests/ref/ranging_ref.c along a unit direction, the statuses, and the C ABI's argument checks
without a device."""
import json
import os

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import duals_ref as D
from tests import parametric_ref as P
from tests import ranging_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))


def _value(A, b, c, basis, d, t):
    """c_B . B^-1 (b + t d) by numpy (the yardstick of a segment's line)."""
    B = A[:, basis]
    return float(c[basis] @ np.linalg.solve(B, b + t * d))


def _paths():
    for name, (A, b, c, basis, d, mx) in sorted(P.named_cases().items()):
        yield name, A, b, c, basis, d, mx, P.parametric(A, b, c, basis, d, np.inf, mx)


def test_golden_objectives_match_highs():
    cases = json.load(open(os.path.join(HERE, "golden", "parametric_cases.json")))
    named = P.named_cases()
    assert len(cases) == len(named)
    checked = 0
    for g in cases:
        A, b, c, basis, d, mx = named[g["name"]]
        r = P.parametric(A, b, c, basis, d, np.inf, mx)
        assert r["status"] == g["status"] and r["nseg"] == g["nseg"]
        ns = r["nseg"]
        for q, (t, z) in enumerate(zip(g["points"], g["objectives"])):
            if q >= ns:   # just past an infeasible end
                assert r["status"] == P.INFEASIBLE and z is None
                continue
            assert z is not None
            line = r["obj"][q] + r["slope"][q] * (t - r["t"][q])
            assert abs(line - z) <= 1e-9 * max(1.0, abs(z)), (g["name"], q, line, z)
            checked += 1
    assert checked >= 50


def test_values_lie_on_each_segment_and_the_path_is_continuous():
    for name, A, b, c, basis, d, mx, r in _paths():
        ns = r["nseg"]
        assert 1 <= ns <= 65
        t, obj, slope = r["t"], r["obj"], r["slope"]
        assert t[0] == 0.0 and (np.diff(t[:ns + 1]) >= 0).all(), name
        for k in range(ns):
            if t[k + 1] == np.inf:
                assert obj[k + 1] == (obj[k] if slope[k] == 0 else np.sign(slope[k]) * np.inf)
                continue
            z = obj[k] + slope[k] * (t[k + 1] - t[k])
            tol = 1e-9 * max(1.0, abs(obj[k + 1]), abs(slope[k]) * (t[k + 1] - t[k]))
            assert abs(z - obj[k + 1]) <= tol, (name, k)
        # both bases at a breakpoint give the same value: replay the bases with numpy
        bases = [np.asarray(basis)]
        for k in range(ns - 1):
            nb = bases[-1].copy()
            nb[list(nb).index(r["leave"][k])] = r["enter"][k]
            bases.append(nb)
        assert np.array_equal(bases[-1], r["basis"]), name
        for k in range(1, ns):
            left, right = _value(A, b, c, bases[k - 1], d, t[k]), _value(A, b, c, bases[k], d, t[k])
            assert abs(left - right) <= 1e-8 * max(1.0, abs(left)), (name, k)
            assert abs(right - obj[k]) <= 1e-8 * max(1.0, abs(right)), (name, k)


def test_slopes_are_monotone_by_sense():
    for name, A, b, c, basis, d, mx, r in _paths():
        s = r["slope"][:r["nseg"]]
        tol = 1e-9 * (1.0 + np.abs(s[:-1]))
        if mx:
            assert (s[1:] <= s[:-1] + tol).all(), name   # concave
        else:
            assert (s[1:] >= s[:-1] - tol).all(), name   # convex


def test_first_slope_is_y_dot_d():
    for name, A, b, c, basis, d, mx, r in _paths():
        y = D.duals(A, b, c, basis)["y"]
        yd = float(y @ d)
        assert abs(r["slope"][0] - yd) <= 1e-9 * max(1.0, np.abs(y).sum() * np.abs(d).max()), name


def test_zero_length_segment_and_outcomes():
    named = P.named_cases()
    z = P.parametric(*named["zero_length"][:5], np.inf, True)
    assert z["nseg"] >= 3 and z["t"][1] == z["t"][2] == 1.0
    assert z["leave"][0] == 0 and z["enter"][0] == 2   # the first position of the tie leaves, y enters
    assert P.parametric(*named["infeasible_end"][:5], np.inf, True)["status"] == P.INFEASIBLE
    u = P.parametric(*named["unbounded_t"][:5], np.inf, True)
    assert u["status"] == P.OPTIMAL and u["t"][u["nseg"]] == np.inf and u["obj"][u["nseg"]] == np.inf
    A, b, c, basis, d, mx = named["max_16x40"]
    full = P.parametric(A, b, c, basis, d, np.inf, mx)
    tm = 0.5 * (full["t"][2] + full["t"][3])
    mid = P.parametric(A, b, c, basis, d, tm, mx)
    assert mid["status"] == P.OPTIMAL and mid["nseg"] == 3 and mid["t"][3] == tm and mid["leave"][2] == -1
    assert np.array_equal(mid["t"][:3], full["t"][:3]) and np.isnan(mid["t"][4:]).all()
    lim = P.parametric(A, b, c, basis, d, np.inf, mx, max_breaks=2)
    assert lim["status"] == P.ITER_LIMIT and lim["nseg"] == 3 and lim["enter"][2] == -1
    assert lim["leave"][2] == full["leave"][2] and lim["t"][3] == full["t"][3]
    zero = P.parametric(A, b, c, basis, d, 0.0, mx)
    assert zero["status"] == P.OPTIMAL and zero["nseg"] == 1 and zero["t"][1] == 0.0


def _ranging_cases():
    """Non-degenerate optimal bases that are not the slack identity: gen_lp (max) and min_lp (min)."""
    out = []
    for seed in range(12):
        A, b, c, basis, _, mx = P.max_case(40 + seed, 4 + seed % 9, 12 + 2 * seed)
        out.append((A, b, c, basis, mx))
        A, b, c, basis, _, mx = P.min_case(40 + seed, 3 + seed % 7, 5 + seed)
        out.append((A, b, c, basis, mx))
    return out


def test_unit_directions_match_ranging_bit_for_bit():
    checked = 0
    for A, b, c, basis, mx in _ranging_cases():
        m, n = A.shape
        rg = RR.ranging(A, b, c, basis, mx)
        assert rg["status"] == 0
        xb = np.linalg.solve(A[:, basis], b)
        if (np.abs(xb) < 1e-7).any():
            continue   # degenerate: tau clamps at 0
        for i in range(m):
            e = np.zeros(m)
            e[i] = 1.0
            up = P.parametric(A, b, c, basis, e, np.inf, mx)
            if rg["b_hi"][i] == np.inf:
                assert up["nseg"] == 1 and up["status"] == P.OPTIMAL
            else:
                assert np.float64(b[i] + up["t"][1]).view(np.uint64) == np.float64(rg["b_hi"][i]).view(np.uint64)
                assert up["leave"][0] == rg["b_leave"][i, 1]
            down = P.parametric(A, b, c, basis, -e, np.inf, mx)
            if rg["b_lo"][i] == -np.inf:
                assert down["nseg"] == 1 and down["status"] == P.OPTIMAL
            else:
                assert np.float64(b[i] - down["t"][1]).view(np.uint64) == np.float64(rg["b_lo"][i]).view(np.uint64)
                assert down["leave"][0] == rg["b_leave"][i, 0]
            checked += 1
    assert checked >= 100


def test_statuses_of_the_reference():
    A, b, c, basis, d, mx = P.named_cases()["max_8x20"]
    m, n = A.shape
    assert P.parametric(A, b, c, basis, d, -1.0, mx)["status"] == P.BAD_ARG
    assert P.parametric(A, b, c, basis, d, np.nan, mx)["status"] == P.BAD_ARG
    assert P.parametric(A, b, c, basis, d, np.inf, mx, eps=-1.0)["status"] == P.BAD_ARG
    bad = basis.copy()
    bad[0] = n
    r = P.parametric(A, b, c, bad, d, np.inf, mx)
    assert r["status"] == P.BAD_ARG and r["nseg"] == 0 and np.isnan(r["t"]).all() and (r["enter"] == -1).all()
    rep = basis.copy()
    rep[1] = rep[0]
    r = P.parametric(A, b, c, rep, d, np.inf, mx)
    assert r["status"] == P.SINGULAR and r["nseg"] == 0 and np.array_equal(r["basis"], rep)
    slack = np.arange(n - m, n, dtype=np.int32)   # the starting basis: primal but not dual feasible
    assert P.parametric(A, b, c, slack, d, np.inf, mx)["status"] == P.BAD_ARG


def test_capi_argument_checks_without_a_device():
    lib = capi.load()
    nseg = np.zeros(1, np.int32)
    t = np.zeros(4)
    ii = np.zeros(4, np.int32)
    dp = t.ctypes.data_as(capi._dp)
    ip = ii.ctypes.data_as(capi._ip)
    np_ = nseg.ctypes.data_as(capi._ip)
    assert lib.lp_basis_parametric(None, dp, 1, 1, dp, dp, ip, 1, dp, 0.0, 0.0, 1, np_, dp, dp, dp, ip, ip, ip) == 5
    assert lib.lp_basis_parametric_batched(None, 1, dp, 1, 1, dp, dp, ip, 1, dp, 0.0, 0.0, 1, np_, dp, dp, dp, ip,
                                           ip, ip, ip) == 5
    assert lib.lp_batched_parametric(None, dp, 0.0, 0.0, 1, np_, dp, dp, dp, ip, ip, ip, ip) == 5
    assert lib.lp_basis_parametric_fits(64, 192) == 1
    assert lib.lp_basis_parametric_fits(512, 1024) == 0
    assert lib.lp_basis_parametric_fits(0, 10) == 0 and lib.lp_basis_parametric_fits(10, 5) == 0
