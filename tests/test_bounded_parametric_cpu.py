"""CPU-only checks of the parametric right-hand-side and cost paths of bounded-variable LPs: the definition
(tests/ref/bounded_parametric_ref.c) against truth it shares no code with.  The identity with tests/ref/parametric_ref.c
and parametric_cost_ref.c at lo = 0, hi = inf; cold solves by tests/ref/bounded_ref.c and HiGHS objectives (the golden
file) at both ends and the midpoint of every segment; the shape of z* (continuity, monotone slopes, t non-decreasing);
the end state re-solved by tests/ref/bounded_resolve_ref.c; one named case per behaviour; every refusal; what the
random set covers; and the fits predicates against the kernel's LDS carve (host calls).  The tolerances are those of
tests/test_parametric_cpu.py and tests/test_parametric_cost_cpu.py for the same comparisons."""
import functools
import json
import os

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_parametric_ref as R
from tests import bounded_ref as B
from tests import bounded_resolve_ref as BR
from tests import parametric_cost_ref as PC
from tests import parametric_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((6, 14, 24), (12, 30, 12))   # m, n, random cases per path
SHARED = ("status", "nseg", "t", "obj", "slope", "enter", "leave", "basis")


@functools.lru_cache(maxsize=None)
def random_paths(path):
    """[(case, full path)] of the random boxed cases of both shapes, both senses in turn; computed once."""
    out = []
    for m, n, count in SHAPES:
        for case in R.random_cases(path, m, n, count):
            out.append((case, R.parametric(path, *case[:8], maximize=case[8])))
    return out


def at_t(path, case, t):
    """(b, c) of the case at parameter t."""
    A, b, c, lo, hi, basis, up, direction, mx = case
    return (b + t * direction, c) if path == "rhs" else (b, c + t * direction)


def samples(r):
    """(segment, t) at both ends and the midpoint of every segment (t_k + 1 + |t_k| inside one that ends at +inf)."""
    for k in range(r["nseg"]):
        t0, t1 = r["t"][k], r["t"][k + 1]
        yield k, t0
        yield k, (t0 + 1.0 + abs(t0)) if t1 == np.inf else 0.5 * (t0 + t1)
        if t1 != np.inf:
            yield k, t1


# ---- the identity ----------------------------------------------------------------------------------------------------

def _plain(path):
    return PR.parametric if path == "rhs" else PC.parametric_cost


def _identity(path, plain_case, settings=((np.inf, 64), (0.75, 64), (np.inf, 2), (np.inf, 0))):
    A, b, c, basis, direction, mx = plain_case
    boxed = R.plain_as_boxed(plain_case)
    for t_max, mb in settings:
        want = _plain(path)(A, b, c, basis, direction, t_max, mx, 1e-9, mb)
        got = R.parametric(path, *boxed[:8], t_max=t_max, maximize=mx, max_breaks=mb)
        R.same_bits(got, want, SHARED)
        assert (got["side"][got["leave"] >= 0] == 0).all() and (got["side"][got["leave"] < 0] == -1).all()
        assert not got["at_upper"].any()


def test_identity_on_the_plain_named_cases():
    cases = R.plain_named_cases()
    assert len(cases) >= 12
    for path, name, plain_case, _ in cases:
        _identity(path, plain_case)


@pytest.mark.parametrize("path", R.PATHS)
def test_identity_on_random_cases_of_both_senses(path):
    mod = PR if path == "rhs" else PC
    for seed in range(1, 9):
        _identity(path, mod.max_case(seed, 6 + seed, 16 + 3 * seed))
        _identity(path, mod.min_case(seed, 5 + seed, 8 + seed))
    # a basis that is not optimal, a repeated index, an index out of range: the same refusals
    A, b, c, basis, direction, mx = mod.max_case(3, 8, 20)
    n = A.shape[1]
    for bad in (np.arange(n - 8, n), np.r_[basis[0], basis[:-1]][[0, 0] + list(range(2, 8))], np.r_[n, basis[1:]]):
        want = _plain(path)(A, b, c, bad.astype(np.int32), direction, np.inf, mx)
        got = R.parametric(path, A, b, c, np.zeros(n), np.full(n, np.inf), bad, np.zeros(n, np.int32), direction,
                           maximize=mx)
        R.same_bits(got, want, SHARED)
        assert got["nseg"] == 0 and (got["side"] == -1).all()


# ---- against cold solves ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", R.PATHS)
def test_every_segment_against_cold_solves(path):
    checked = 0
    for case, r in random_paths(path):
        A, b, c, lo, hi, basis, up, direction, mx = case
        for k, t in samples(r):
            bt, ct = at_t(path, case, t)
            cold = B.bounded(A, bt, ct, lo, hi, mx)
            assert cold["status"] == R.OPTIMAL, (k, t)
            z = cold["obj"]
            line = r["obj"][k] + r["slope"][k] * (t - r["t"][k])
            assert abs(line - z) <= 1e-9 * max(1.0, abs(z)), (path, k, t, line, z)
            checked += 1
        if r["status"] in (R.INFEASIBLE, R.UNBOUNDED):   # just past the end the cold solve agrees with the verdict
            te = r["t"][r["nseg"]]
            bt, ct = at_t(path, case, te + 0.05 * (1.0 + abs(te)))
            assert B.bounded(A, bt, ct, lo, hi, mx)["status"] == r["status"]
    assert checked >= 500


def test_golden_objectives_match_highs():
    cases = json.load(open(os.path.join(HERE, "golden", "bounded_parametric_cases.json")))
    assert len(cases) >= 24 and {g["args"]["path"] for g in cases} == set(R.PATHS)
    checked = 0
    for g in cases:
        case = R.boxed_case(**g["args"])
        path = g["args"]["path"]
        r = R.parametric(path, *case[:8], maximize=case[8])
        assert r["status"] == g["status"] and r["nseg"] == g["nseg"], g["args"]
        for t, k, z in zip(g["points"], g["segment"], g["objectives"]):
            if k >= r["nseg"]:   # just past an infeasible or unbounded end
                assert r["status"] in (R.INFEASIBLE, R.UNBOUNDED) and z is None
                continue
            assert z is not None, (g["args"], t)
            line = r["obj"][k] + r["slope"][k] * (t - r["t"][k])
            assert abs(line - z) <= 1e-9 * max(1.0, abs(z)), (g["args"], k, t, line, z)
            checked += 1
    assert checked >= 500


# ---- the shape of z* --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", R.PATHS)
def test_continuity_monotone_slopes_and_t(path):
    for case, r in random_paths(path):
        mx = case[8]
        ns = r["nseg"]
        t, obj, slope = r["t"], r["obj"], r["slope"]
        assert 1 <= ns <= 65 and t[0] == 0.0 and not np.signbit(t[0]) and (np.diff(t[:ns + 1]) >= 0).all()
        for k in range(ns):
            if t[k + 1] == np.inf:
                assert obj[k + 1] == (obj[k] if slope[k] == 0 else np.sign(slope[k]) * np.inf)
                continue
            z = obj[k] + slope[k] * (t[k + 1] - t[k])
            tol = 1e-9 * max(1.0, abs(obj[k + 1]), abs(slope[k]) * (t[k + 1] - t[k]))
            assert abs(z - obj[k + 1]) <= tol, (path, k)
        s = slope[:ns]
        tol = 1e-9 * (1.0 + np.abs(s[:-1]))
        # RHS: concave for max, convex for min; cost: convex for max, concave for min
        if mx == (path == "rhs"):
            assert (s[1:] <= s[:-1] + tol).all(), path
        else:
            assert (s[1:] >= s[:-1] - tol).all(), path


# ---- the end state ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", R.PATHS)
def test_the_returned_basis_and_flags_are_optimal_at_a_finite_end(path):
    checked = {R.OPTIMAL: 0, R.ITER_LIMIT: 0}
    for case, _ in random_paths(path):
        A, b, c, lo, hi, basis, up, direction, mx = case
        for t_max, mb in ((0.3, 64), (np.inf, 3), (2.0, 64)):
            r = R.parametric(path, *case[:8], t_max=t_max, maximize=mx, max_breaks=mb)
            te = r["t"][r["nseg"]]
            if r["status"] not in checked or te == np.inf:
                continue
            bt, ct = at_t(path, case, te)
            warm = BR.resolve(A, bt, ct, lo, hi, r["basis"], r["at_upper"], mx)
            assert warm["status"] == R.OPTIMAL and warm["iters"] == [0, 0, 0], (path, t_max, mb)
            assert np.array_equal(warm["basis"], r["basis"]) and np.array_equal(warm["at_upper"], r["at_upper"])
            assert abs(warm["obj"] - r["obj"][r["nseg"]]) <= 1e-9 * max(1.0, abs(warm["obj"]))
            checked[r["status"]] += 1
    assert checked[R.OPTIMAL] >= 20 and checked[R.ITER_LIMIT] >= 20


# ---- named cases, one per behaviour -----------------------------------------------------------------------------------

def _named(name, **more):
    path, args, kw, status = R.named_cases()[name]
    r = R.parametric(path, *args[:8], maximize=args[8], **dict(kw, **more))
    assert status is None or r["status"] == status, name
    return args, r, R.trim(r)


def test_named_rhs_blocked_at_an_upper_bound():
    (A, b, c, lo, hi, *_), r, tr = _named("rhs_upper_blocked")
    assert tr["status"] == R.OPTIMAL and tr["leave"][0] == 0 and tr["side"][0] == 1 and tr["t"][1] == 1.5
    assert tr["at_upper"][0] == 1 and 0 not in tr["basis"]          # x0 now sits at hi = 3
    assert tr["obj"].tolist() == [6.5, 8.0, 8.0] and tr["slope"].tolist() == [1.0, 0.0]


def test_named_cost_flip_and_leave_at_upper():
    (A, b, c, lo, hi, *_), r, tr = _named("cost_flip")
    flips = (tr["enter"] == tr["leave"]) & (tr["enter"] >= 0)
    assert flips.any() and (hi[tr["enter"][flips]] > lo[tr["enter"][flips]]).any()
    _, r, tr = _named("cost_fixed_flip")                          # a fixed column flips in place: nothing moves
    k = int(np.flatnonzero((tr["enter"] == tr["leave"]) & (tr["enter"] >= 0))[0])
    assert tr["enter"][k] == 2 and tr["side"][k] == 0 and tr["slope"][k + 1] == tr["slope"][k]
    _, r, tr = _named("cost_leave_at_upper")
    pivots = (tr["enter"] != tr["leave"]) & (tr["leave"] >= 0)
    assert (tr["side"][pivots] == 1).any()
    k = int(np.flatnonzero(pivots & (tr["side"] == 1))[0])
    assert tr["t"][k + 1] > 0
    # random flips: the flag of the flipped column is the recorded side when the path ends there
    for case, full in random_paths("cost"):
        for k in range(full["nseg"] - 1):
            if full["enter"][k] == full["leave"][k]:
                stop = R.parametric("cost", *case[:8], maximize=case[8], max_breaks=k + 1)
                assert stop["at_upper"][full["enter"][k]] == full["side"][k]


def test_named_ends():
    _, r, tr = _named("rhs_infeasible_end")
    assert tr["leave"][-1] >= 0 and tr["enter"][-1] == -1 and tr["side"][-1] in (0, 1) and np.isfinite(tr["t"][-1])
    _, r, tr = _named("cost_unbounded_end")
    assert tr["enter"][-1] == 5 and tr["leave"][-1] == -1 and tr["side"][-1] == -1 and tr["t"][-1] == 1.0
    for name in ("rhs_tmax_inside", "cost_tmax_inside"):
        _, r, tr = _named(name)
        assert tr["t"][-1] == 0.75 and len(tr["slope"]) == 1 and tr["enter"][-1] == tr["leave"][-1] == -1
        assert tr["obj"][-1] == tr["obj"][0] + 0.75 * tr["slope"][0]
    _, r, tr = _named("rhs_end_at_inf")
    assert tr["t"][-1] == np.inf and tr["slope"][-1] == 0.0 and tr["obj"][-1] == tr["obj"][-2]
    _, r, tr = _named("cost_end_at_inf")
    assert tr["t"][-1] == np.inf and tr["slope"][-1] > 0 and tr["obj"][-1] == np.inf
    for name in ("rhs_iter_limit", "cost_iter_limit"):
        _, r, tr = _named(name)
        assert len(tr["slope"]) == 1 and np.isfinite(tr["t"][-1]) and tr["t"][-1] > 0
        assert (tr["leave"][-1] >= 0) == name.startswith("rhs") and (tr["enter"][-1] >= 0) == name.startswith("cost")
        args = R.named_cases()[name][1]
        assert np.array_equal(tr["basis"], args[5]) and np.array_equal(tr["at_upper"], args[6])   # no trace


def test_named_zero_length_and_fixed_basic():
    _, r, tr = _named("rhs_zero_length")
    assert len(tr["slope"]) >= 3 and tr["t"][1] == tr["t"][2] == 1.0 and tr["obj"][1] == tr["obj"][2]
    for name in ("rhs_fixed_basic", "cost_fixed_basic"):
        (A, b, c, lo, hi, basis, *_), r, tr = _named(name)
        assert lo[1] == hi[1] and 1 in basis
        assert tr["leave"][0] == 1 and tr["t"][1] == 0.0 and tr["status"] == R.OPTIMAL   # it leaves at once
        assert np.isfinite(tr["obj"][:-1]).all()


def test_named_outcomes_without_a_path():
    for name in ("crossed", "cost_crossed", "singular", "cost_singular", "start_dual_infeasible",
                 "start_primal_infeasible"):
        args, r, tr = _named(name)
        assert r["nseg"] == 0 and np.isnan(r["t"]).all() and np.isnan(r["obj"]).all() and np.isnan(r["slope"]).all()
        assert (r["enter"] == -1).all() and (r["leave"] == -1).all() and (r["side"] == -1).all()
        assert np.array_equal(r["basis"], args[5]) and np.array_equal(r["at_upper"], args[6])


@pytest.mark.parametrize("path", R.PATHS)
def test_each_refusal(path):
    A, b, c, lo, hi, basis, up, direction, mx = R.named_cases()["rhs_upper_blocked" if path == "rhs" else "cost_fixed_flip"][1]
    n = A.shape[1]
    free = int(np.flatnonzero(np.isinf(hi))[0])

    def run(t_max=np.inf, eps=1e-9, max_breaks=8, **kw):
        a = dict(lo=lo, hi=hi, basis=basis, up=up)
        a.update(kw)
        return R.parametric(path, A, b, c, a["lo"], a["hi"], a["basis"], a["up"], direction, t_max, mx, eps, max_breaks)

    def with_(v, at, val):
        v = np.array(v, dtype=np.float64 if np.asarray(v).dtype.kind == "f" else np.int32)
        v[at] = val
        return v

    assert run()["status"] == R.OPTIMAL
    refused = [run(lo=with_(lo, 1, np.nan)), run(lo=with_(lo, 1, -np.inf)), run(lo=with_(lo, 1, np.inf)),
               run(hi=with_(hi, 1, np.nan)), run(up=with_(up, 2, 2)), run(up=with_(up, 2, -1)),
               run(up=with_(np.zeros(n, np.int32), free, 1)), run(basis=with_(basis, 0, n)),
               run(basis=with_(basis, 0, -1)), run(t_max=-1.0), run(t_max=np.nan), run(eps=-1.0), run(eps=np.nan)]
    for r in refused:
        assert r["status"] == R.BAD_ARG and r["nseg"] == 0 and np.isnan(r["t"]).all() and (r["side"] == -1).all()
    assert run(max_breaks=-1)["status"] == R.BAD_ARG
    assert run(hi=with_(hi, 0, lo[0] - 0.5))["status"] == R.INFEASIBLE
    assert run(hi=with_(hi, 0, -np.inf))["status"] == R.INFEASIBLE
    assert run(hi=with_(hi, 0, lo[0] - 0.5), basis=with_(basis, 1, basis[0]))["status"] == R.INFEASIBLE   # crossed first
    assert run(hi=with_(hi, 0, lo[0] - 0.5), t_max=-1.0)["status"] == R.BAD_ARG                           # the checks first
    assert run(basis=with_(basis, 1, basis[0]))["status"] == R.SINGULAR
    # NULL pointers, straight at the library
    L = R.lib()
    fn = L.ref_bounded_parametric if path == "rhs" else L.ref_bounded_parametric_cost
    Af = np.ascontiguousarray(A.T).reshape(-1)
    m = A.shape[0]
    ii = [np.zeros(k, np.int32) for k in (1, 9, 9, 9, m, n)]
    dd = [np.zeros(10), np.zeros(10), np.zeros(9)]
    good = [R._d(Af), m, n, R._d(b), R._d(c), R._d(lo), R._d(hi), R._i(np.asarray(basis, np.int32)),
            R._i(np.asarray(up, np.int32)), 1, R._d(direction), np.inf, 1e-9, 8, R._i(ii[0]), R._d(dd[0]), R._d(dd[1]),
            R._d(dd[2]), R._i(ii[1]), R._i(ii[2]), R._i(ii[3]), R._i(ii[4]), R._i(ii[5])]
    assert fn(*good) == R.OPTIMAL
    for pos in (0, 3, 4, 5, 6, 7, 8, 10, 14, 15, 16, 17, 18, 19, 20, 21, 22):
        bad = list(good)
        bad[pos] = None
        assert fn(*bad) == R.BAD_ARG, pos


# ---- what the random set covers ---------------------------------------------------------------------------------------

def test_the_random_set_covers_every_behaviour():
    rhs, cost = random_paths("rhs"), random_paths("cost")
    assert {case[8] for case, _ in rhs} == {True, False} == {case[8] for case, _ in cost}
    assert any((r["side"][:r["nseg"]] == 1).any() for _, r in rhs)                       # blocked at an upper bound
    assert any((r["enter"][:r["nseg"] - 1] == r["leave"][:r["nseg"] - 1]).any() for _, r in cost)   # a bound flip
    piv = [(r["enter"] != r["leave"]) & (r["leave"] >= 0) & (r["side"] == 1) for _, r in cost]
    assert any(p.any() for p in piv)                                                     # a pivot that leaves at hi
    assert any(r["status"] == R.INFEASIBLE for _, r in rhs) and any(r["status"] == R.UNBOUNDED for _, r in cost)
    assert any(r["status"] == R.OPTIMAL for _, r in cost)
    for paths in (rhs, cost):
        hi_kinds = set()
        for case, _ in paths:
            lo, hi = case[3], case[4]
            hi_kinds |= {"inf"} if np.isinf(hi).any() else set()
            hi_kinds |= {"finite"} if (np.isfinite(hi) & (hi > lo)).any() else set()
            hi_kinds |= {"fixed"} if (hi == lo).any() else set()
        assert hi_kinds == {"inf", "finite", "fixed"}


# ---- the fits predicates (host calls) ---------------------------------------------------------------------------------

def carve_bytes(m, n, cost):
    """The LDS carve of the two kernels, restated: batched_bounded_carve.hpp's for (m, n + 1) or (m + 1, n), then the
    segment's end (2 doubles), hi, c (and g) and the held values, the slot of every column and 4 published ints."""
    mm, nn = (m + 1, n) if cost else (m, n + 1)
    W = nn + 1
    pitch = W | 1
    o = 16 + 8 * ((mm + 1) * pitch + W + (mm + 1) + 2 * nn) + 4 * (2 * nn + mm)
    o = (o + 15) & ~15
    o += 8 * (2 + (4 if cost else 3) * n) + 4 * (n + 4)
    return (o + 15) & ~15


def test_fits_at_and_just_past_the_edge():
    lib = capi.load()
    for cost, fits in ((False, lib.lp_basis_bounded_parametric_fits), (True, lib.lp_basis_bounded_parametric_cost_fits)):
        assert fits(64, 192) == 1 and carve_bytes(64, 192, cost) <= 160 * 1024
        assert fits(8, 20) == 1 and fits(0, 4) == 0 and fits(4, 3) == 0 and fits(-1, -1) == 0
        for m in list(range(1, 150)) + [180, 200]:
            for n in (m, m + 1, m + 7, 2 * m, 3 * m, 8 * m, 40 * m):
                want = lib.lp_simplex_bounded_fits(m, n) == 1 and carve_bytes(m, n, cost) <= 160 * 1024
                assert fits(m, n) == int(want), (cost, m, n)
        # both sides of the limit along n at m = 64 and along m = n
        n = 192
        while fits(64, n + 1):
            n += 1
        assert carve_bytes(64, n, cost) <= 160 * 1024 < carve_bytes(64, n + 1, cost) and n >= 256
        m = 64
        while fits(m + 1, m + 1):
            m += 1
        assert carve_bytes(m, m, cost) <= 160 * 1024 < carve_bytes(m + 1, m + 1, cost)
        assert lib.lp_simplex_bounded_fits(64, n + 1) == 1 and lib.lp_simplex_bounded_fits(m + 1, m + 1) == 1


def test_capi_argument_checks_without_a_device():
    lib = capi.load()
    t, ii = np.zeros(4), np.zeros(4, np.int32)
    dp, ip = t.ctypes.data_as(capi._dp), ii.ctypes.data_as(capi._ip)
    for fn in (lib.lp_basis_bounded_parametric, lib.lp_basis_bounded_parametric_cost):
        assert fn(None, dp, 1, 1, dp, dp, dp, dp, ip, ip, 1, dp, 0.0, 0.0, 1, ip, dp, dp, dp, ip, ip, ip, ip, ip) == 5
    for fn in (lib.lp_basis_bounded_parametric_batched, lib.lp_basis_bounded_parametric_cost_batched):
        assert fn(None, 1, dp, 1, 1, dp, dp, dp, dp, ip, ip, None, 1, dp, 0.0, 0.0, 1, ip, dp, dp, dp, ip, ip, ip, ip,
                  ip, ip) == 5
