"""CPU-only checks of the parametric cost path: the test restatement (tests/ref/parametric_cost_ref.c) against HiGHS
objectives at every breakpoint and segment midpoint (the golden cases) and HiGHS's unbounded verdict past every
UNBOUNDED end, the path's own algebra (continuity at every breakpoint, convex for max and concave for min, each slope
as g.x of its segment's basic solution), agreement with the cost ranging of tests/ref/ranging_ref.c along a unit
direction, the statuses and padding, and the C ABI's argument checks without a device."""
import json
import os

import numpy as np

from simplexmethod_amd import capi
from tests import parametric_cost_ref as P
from tests import ranging_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))


def _x(A, b, basis):
    """The basic solution of `basis` by numpy."""
    x = np.zeros(A.shape[1])
    x[basis] = np.linalg.solve(A[:, basis], b)
    return x


def _paths():
    for name, (A, b, c, basis, g, mx) in sorted(P.named_cases().items()):
        yield name, A, b, c, basis, g, mx, P.parametric_cost(A, b, c, basis, g, np.inf, mx)


def _bases(basis, r):
    """The basis of every segment, replayed from the start basis and the enter / leave sequence."""
    out = [np.asarray(basis)]
    for k in range(r["nseg"] - 1):
        nb = out[-1].copy()
        nb[list(nb).index(r["leave"][k])] = r["enter"][k]
        out.append(nb)
    return out


def test_golden_objectives_match_highs():
    cases = json.load(open(os.path.join(HERE, "golden", "parametric_cost_cases.json")))
    named = P.named_cases()
    assert len(cases) == len(named)
    checked = unbounded = 0
    for gc in cases:
        A, b, c, basis, g, mx = named[gc["name"]]
        r = P.parametric_cost(A, b, c, basis, g, np.inf, mx)
        assert r["status"] == gc["status"] and r["nseg"] == gc["nseg"]
        ns = r["nseg"]
        for t, k, z in zip(gc["points"], gc["segment"], gc["objectives"]):
            if k >= ns:   # just past an unbounded end
                assert r["status"] == P.UNBOUNDED and z is None
                unbounded += 1
                continue
            assert z is not None
            line = r["obj"][k] + r["slope"][k] * (t - r["t"][k])
            assert abs(line - z) <= 1e-9 * max(1.0, abs(z)), (gc["name"], k, t, line, z)
            checked += 1
    assert checked >= 100 and unbounded >= 3


def test_path_is_continuous_and_bases_agree_at_breakpoints():
    for name, A, b, c, basis, g, mx, r in _paths():
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
        bases = _bases(basis, r)
        assert np.array_equal(bases[-1], r["basis"]), name
        for k in range(1, ns):   # both bases at a breakpoint give the same value
            cost = c + t[k] * g
            left, right = cost @ _x(A, b, bases[k - 1]), cost @ _x(A, b, bases[k])
            assert abs(left - right) <= 1e-8 * max(1.0, abs(left)), (name, k)
            assert abs(right - obj[k]) <= 1e-8 * max(1.0, abs(right)), (name, k)


def test_slopes_are_monotone_by_sense():
    for name, A, b, c, basis, g, mx, r in _paths():
        s = r["slope"][:r["nseg"]]
        tol = 1e-9 * (1.0 + np.abs(s[:-1]))
        if mx:
            assert (s[1:] >= s[:-1] - tol).all(), name   # convex
        else:
            assert (s[1:] <= s[:-1] + tol).all(), name   # concave


def test_slope_is_g_dot_x_of_each_segment():
    for name, A, b, c, basis, g, mx, r in _paths():
        for k, B in enumerate(_bases(basis, r)):
            gx = float(g @ _x(A, b, B))
            assert abs(r["slope"][k] - gx) <= 1e-9 * max(1.0, np.abs(g).sum() * np.abs(b).max()), (name, k)


def test_outcomes_of_the_named_cases():
    named = P.named_cases()
    for mx in (True, False):
        sfx = "max" if mx else "min"
        z = P.parametric_cost(*named["zero_length_" + sfx][:5], np.inf, mx)
        assert z["status"] == P.OPTIMAL and z["nseg"] == 3 and z["t"][1] == z["t"][2] == 1.0
        assert list(z["enter"][:3]) == [2, 3, -1] and list(z["leave"][:3]) == [0, 1, -1]
        assert z["obj"][3] == (np.inf if mx else -np.inf)
        u = P.parametric_cost(*named["unbounded_" + sfx][:5], np.inf, mx)
        assert u["status"] == P.UNBOUNDED and u["nseg"] == 1 and u["t"][1] == 1.0
        assert u["enter"][0] == 2 and u["leave"][0] == -1
    zg = P.parametric_cost(*named["zero_g"][:5], np.inf, True)
    assert zg["status"] == P.OPTIMAL and zg["nseg"] == 1 and zg["slope"][0] == 0.0
    assert zg["t"][1] == np.inf and zg["obj"][1] == zg["obj"][0] and np.isfinite(zg["obj"][1])
    assert P.parametric_cost(*named["min_12x32_unbounded"][:5], np.inf, False)["status"] == P.UNBOUNDED
    for name in ("max_8x20", "min_6x16_inf"):
        A, b, c, basis, g, mx = named[name]
        r = P.parametric_cost(A, b, c, basis, g, np.inf, mx)
        assert r["status"] == P.OPTIMAL and r["nseg"] >= 3 and r["t"][r["nseg"]] == np.inf
        assert r["slope"][r["nseg"] - 1] != 0.0 and abs(r["obj"][r["nseg"]]) == np.inf
    A, b, c, basis, g, mx = named["max_16x40"]
    full = P.parametric_cost(A, b, c, basis, g, np.inf, mx)
    tm = 0.5 * (full["t"][2] + full["t"][3])
    mid = P.parametric_cost(A, b, c, basis, g, tm, mx)
    assert mid["status"] == P.OPTIMAL and mid["nseg"] == 3 and mid["t"][3] == tm and mid["enter"][2] == -1
    assert np.array_equal(mid["t"][:3], full["t"][:3]) and np.isnan(mid["t"][4:]).all()
    assert (mid["enter"][3:] == -1).all() and np.isnan(mid["slope"][3:]).all()
    lim = P.parametric_cost(A, b, c, basis, g, np.inf, mx, max_breaks=2)
    assert lim["status"] == P.ITER_LIMIT and lim["nseg"] == 3 and lim["leave"][2] == -1
    assert lim["enter"][2] == full["enter"][2] and lim["t"][3] == full["t"][3]
    assert lim["t"].shape == (4,) and lim["enter"].shape == (3,)
    zero = P.parametric_cost(A, b, c, basis, g, 0.0, mx)
    assert zero["status"] == P.OPTIMAL and zero["nseg"] == 1 and zero["t"][1] == 0.0


def _ranging_cases():
    """Optimal bases of gen_lp (max) that are not the slack identity."""
    out = []
    for seed in range(12):
        A, b, c, basis, _, mx = P.max_case(60 + seed, 4 + seed % 9, 12 + 2 * seed)
        out.append((A, b, c, basis, mx))
    return out


def test_unit_directions_match_cost_ranging():
    checked = 0
    for A, b, c, basis, mx in _ranging_cases():
        m, n = A.shape
        rg = RR.ranging(A, b, c, basis, mx)
        assert rg["status"] == 0
        for j in sorted(set(range(n)) - set(basis.tolist())):
            e = np.zeros(n)
            e[j] = 1.0
            up = P.parametric_cost(A, b, c, basis, e, np.inf, mx)
            assert up["nseg"] >= 1 and up["enter"][0] == j
            hi = rg["c_hi"][j]
            assert abs(c[j] + up["t"][1] - hi) <= 1e-12 * max(1.0, abs(hi)), (j, c[j] + up["t"][1], hi)
            checked += 1
    assert checked >= 100


def test_statuses_and_padding_of_the_reference():
    A, b, c, basis, g, mx = P.named_cases()["max_8x20"]
    m, n = A.shape
    assert P.parametric_cost(A, b, c, basis, g, -1.0, mx)["status"] == P.BAD_ARG
    assert P.parametric_cost(A, b, c, basis, g, np.nan, mx)["status"] == P.BAD_ARG
    assert P.parametric_cost(A, b, c, basis, g, np.inf, mx, eps=-1.0)["status"] == P.BAD_ARG
    assert P.parametric_cost(A, b, c, basis, g, np.inf, mx, eps=np.nan)["status"] == P.BAD_ARG
    assert P.parametric_cost(A, b, c, basis, g, np.inf, mx, max_breaks=-1)["status"] == P.BAD_ARG
    bad = basis.copy()
    bad[0] = n
    r = P.parametric_cost(A, b, c, bad, g, np.inf, mx)
    assert r["status"] == P.BAD_ARG and r["nseg"] == 0 and np.isnan(r["t"]).all() and (r["enter"] == -1).all()
    assert np.array_equal(r["basis"], bad)
    rep = basis.copy()
    rep[1] = rep[0]
    r = P.parametric_cost(A, b, c, rep, g, np.inf, mx)
    assert r["status"] == P.SINGULAR and r["nseg"] == 0 and np.array_equal(r["basis"], rep)
    assert np.isnan(r["obj"]).all() and np.isnan(r["slope"]).all() and (r["leave"] == -1).all()
    slack = np.arange(n - m, n, dtype=np.int32)   # the starting basis: primal but not dual feasible
    r = P.parametric_cost(A, b, c, slack, g, np.inf, mx)
    assert r["status"] == P.BAD_ARG and r["nseg"] == 0 and np.array_equal(r["basis"], slack)
    full = P.parametric_cost(A, b, c, basis, g, np.inf, mx)
    ns = full["nseg"]
    assert np.isnan(full["t"][ns + 1:]).all() and np.isnan(full["obj"][ns + 1:]).all()
    assert np.isnan(full["slope"][ns:]).all() and (full["enter"][ns:] == -1).all() and (full["leave"][ns:] == -1).all()


def test_capi_argument_checks_without_a_device():
    lib = capi.load()
    nseg = np.zeros(1, np.int32)
    t = np.zeros(4)
    ii = np.zeros(4, np.int32)
    dp = t.ctypes.data_as(capi._dp)
    ip = ii.ctypes.data_as(capi._ip)
    np_ = nseg.ctypes.data_as(capi._ip)
    assert lib.lp_basis_parametric_cost(None, dp, 1, 1, dp, dp, ip, 1, dp, 0.0, 0.0, 1, np_, dp, dp, dp, ip, ip,
                                        ip) == 5
    assert lib.lp_basis_parametric_cost_batched(None, 1, dp, 1, 1, dp, dp, ip, 1, dp, 0.0, 0.0, 1, np_, dp, dp, dp,
                                                ip, ip, ip, ip) == 5
    assert lib.lp_batched_parametric_cost(None, dp, 0.0, 0.0, 1, np_, dp, dp, dp, ip, ip, ip, ip) == 5
    assert lib.lp_basis_parametric_cost_fits(64, 192) == 1
    assert lib.lp_basis_parametric_cost_fits(128, 256) == 0
    assert lib.lp_basis_parametric_cost_fits(512, 1024) == 0
    assert lib.lp_basis_parametric_cost_fits(0, 10) == 0 and lib.lp_basis_parametric_cost_fits(10, 5) == 0
