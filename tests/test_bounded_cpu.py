"""The bounded-variable simplex without a GPU: tests/ref/bounded_ref.c against scipy's HiGHS on random boxed LPs (both
senses, fixed, negative-lo and infinite-hi columns, infeasible and unbounded cases), against the same LPs with every
finite upper bound written as a row and slack (pyoracle.two_phase), bit for bit against pyoracle.two_phase with
lo = 0 and hi = inf, and the host-only parts of the C ABI (lp_simplex_bounded_fits, refusals without a context)."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import linprog

from oracle import pyoracle
from simplexmethod_amd import capi
from tests import bounded_ref as R

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = 0, 1, 2, 3, 4, 5
_HIGHS = {0: OPTIMAL, 2: INFEASIBLE, 3: UNBOUNDED}
_KINDS = ("mixed", "mixed", "box", "infeasible", "unbounded", "crossed")


def _case(s):
    m = 3 + s % 8
    n = m + 3 + (7 * s) % 13
    return R.boxed_lp(s, m, n, maximize=s % 2 == 0, kind=_KINDS[s % len(_KINDS)])


def _highs(A, b, c, lo, hi, maximize):
    bounds = [(float(l), None if np.isinf(h) else float(h)) for l, h in zip(lo, hi)]
    if np.any(hi < lo):
        return INFEASIBLE, None
    res = linprog(-c if maximize else c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    return _HIGHS[res.status], (None if res.status else (-res.fun if maximize else res.fun))


@pytest.mark.parametrize("s", range(96))
def test_matches_highs(s):
    A, b, c, lo, hi, mx = _case(s)
    r = R.bounded(A, b, c, lo, hi, mx)
    st, z = _highs(A, b, c, lo, hi, mx)
    assert r["status"] == st
    if st != OPTIMAL:
        assert np.isnan(r["obj"]) and np.all(np.isnan(r["x"]))
        return
    assert abs(r["obj"] - z) <= 1e-7 * max(1.0, abs(z))
    x = r["x"]
    scale = max(1.0, float(np.abs(b).max()))
    assert np.all(np.abs(A @ x - b) <= 1e-9 * scale)
    assert np.all(x >= lo - 1e-9) and np.all(x <= hi + 1e-9)
    assert r["obj"] == float(sum(float(c[j] * x[j]) for j in range(len(x))))   # the objective is c.x in index order
    up = r["at_upper"].astype(bool)
    nonbasic = np.ones(len(x), bool)
    nonbasic[r["basis"]] = False
    assert np.all(x[nonbasic & ~up] == lo[nonbasic & ~up])
    assert np.allclose(x[nonbasic & up], hi[nonbasic & up], rtol=0, atol=1e-12 * scale)


@pytest.mark.parametrize("s", range(96))
def test_matches_the_row_form(s):
    A, b, c, lo, hi, mx = _case(s)
    if np.any(hi < lo):
        return
    r = R.bounded(A, b, c, lo, hi, mx)
    A2, b2, c2, const = R.as_rows(A, b, c, lo, hi)
    q = pyoracle.two_phase(A2, b2, c2, mx)
    assert r["status"] == q["status"]
    if q["status"] == OPTIMAL:
        z = q["obj"] + const
        assert abs(r["obj"] - z) <= 1e-7 * max(1.0, abs(z))


def test_outcomes_are_all_reached():
    seen = {R.bounded(*_case(s)[:5], _case(s)[5])["status"] for s in range(96)}
    assert {OPTIMAL, INFEASIBLE, UNBOUNDED} <= seen
    flips = sum(R.bounded(*_case(s)[:5], _case(s)[5])["iters"][3] for s in range(0, 96, 6))
    assert flips > 0


@pytest.mark.parametrize("seed", range(24))
@pytest.mark.parametrize("maximize", [True, False])
def test_identity_anchor_equals_two_phase(seed, maximize):
    m, n = 4 + seed % 9, 12 + (3 * seed) % 20
    A, b, c, _ = capi.gen_lp(seed, m, n)
    if not maximize:
        c = -c
    if seed % 3 == 0:
        b = b.copy()
        b[::2] *= -1.0
    r = R.bounded(A, b, c, np.zeros(n), np.full(n, np.inf), maximize, n - m)
    q = pyoracle.two_phase(A, b, c, maximize, n - m)
    assert r["status"] == q["status"]
    assert np.array_equal(r["basis"], q["basis"])
    assert r["iters"][:3] == q["iters"] and r["iters"][3] == 0
    assert not r["at_upper"].any()
    if q["status"] == OPTIMAL:
        assert np.array_equal(r["x"], q["x"]) and r["obj"] == q["obj"]


def test_iteration_limit_counts_flips():
    A, b, c, lo, hi, mx = R.boxed_lp(0, 8, 24, kind="box")
    full = R.bounded(A, b, c, lo, hi, mx)
    assert full["status"] == OPTIMAL and full["iters"][3] > 0
    lim = R.bounded(A, b, c, lo, hi, mx, max_iter=1)
    assert lim["status"] == ITER_LIMIT and sum(lim["iters"]) == 1   # one pivot or one flip
    assert R.bounded(A, b, c, lo, hi, mx, max_iter=0)["status"] == ITER_LIMIT


def test_crossed_bounds_are_infeasible_without_iterations():
    A, b, c, lo, hi, mx = R.boxed_lp(2, 5, 14, kind="crossed")
    r = R.bounded(A, b, c, lo, hi, mx)
    assert r["status"] == INFEASIBLE and r["iters"] == [0, 0, 0, 0]
    assert list(r["basis"]) == list(range(14, 19)) and not r["at_upper"].any()


def test_reference_refuses_bad_bounds():
    A, b, c, lo, hi, mx = R.boxed_lp(1, 6, 16)
    assert R.bounded(A, b, c, lo, hi, mx)["status"] == OPTIMAL
    for j, (l, h) in enumerate(((-np.inf, 1.0), (np.nan, 1.0), (np.inf, np.inf), (0.0, np.nan))):
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[j], hi2[j] = l, h
        assert R.bounded(A, b, c, lo2, hi2, mx)["status"] == BAD_ARG


def test_fits_is_a_host_call():
    lib = capi.load()
    assert lib.lp_simplex_bounded_fits(64, 192) == 1
    assert lib.lp_simplex_bounded_fits(32, 96) == 1
    assert lib.lp_simplex_bounded_fits(160, 320) == 0
    assert lib.lp_simplex_bounded_fits(0, 10) == 0 and lib.lp_simplex_bounded_fits(8, 4) == 0


def test_capi_refuses_without_a_context():
    lib = capi.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    z = np.zeros(16)
    zi = np.zeros(16, np.int32)
    d, i = z.ctypes.data_as(dp), zi.ctypes.data_as(ip)
    assert lib.lp_simplex_bounded(None, d, 2, 4, d, d, d, d, 1, 4, 1e-9, 10, d, i, i, d, i) == BAD_ARG
    assert lib.lp_simplex_bounded_batched(None, 1, d, 2, 4, d, d, d, d, 1, 4, 1e-9, 10, d, i, i, d, i, i) == BAD_ARG
