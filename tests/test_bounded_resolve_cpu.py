"""The bounded-variable re-solve without a GPU: tests/ref/bounded_resolve_ref.c, warm-started from
tests/ref/bounded_ref.c's optimum, against scipy's HiGHS after a change of bounds, of b or of c; bit for bit against
tests/ref/resolve_ref.c with lo = 0, hi = inf and no flag; the cold optimum fed back unchanged; every outcome; and the
host-only refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_ref as B
from tests import bounded_resolve_ref as W
from tests import resolve_ref
from tests.test_bounded_cpu import _highs
from tests.test_resolve_cpu import _rhs_changed

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = 0, 1, 2, 3, 4, 5


def _shape(s):   # the 96 shapes of test_bounded_cpu._case
    m = 3 + s % 8
    return m, m + 3 + (7 * s) % 13


def _cold(s, kind):
    m, n = _shape(s)
    A, b, c, lo, hi, mx = B.boxed_lp(s, m, n, maximize=s % 2 == 0, kind=kind)
    return A, b, c, lo, hi, mx, B.bounded(A, b, c, lo, hi, mx)


@pytest.mark.parametrize("pert", W.PERTURBATIONS)
@pytest.mark.parametrize("kind", ["mixed", "box"])
@pytest.mark.parametrize("s", range(96))
def test_matches_highs(s, kind, pert):
    A, b, c, lo, hi, mx, r = _cold(s, kind)
    if r["status"] != OPTIMAL:
        return   # (test_cold_starts_exist counts them)
    b2, c2, lo2, hi2 = W.perturb(s, pert, b, c, lo, hi, r["basis"], r["x"])
    g = W.resolve(A, b2, c2, lo2, hi2, r["basis"], r["at_upper"], mx)
    st, z = _highs(A, b2, c2, lo2, hi2, mx)
    assert g["status"] == st
    if st != OPTIMAL:
        assert np.isnan(g["obj"]) and np.all(np.isnan(g["x"]))
        return
    assert abs(g["obj"] - z) <= 1e-7 * max(1.0, abs(z))
    x = g["x"]
    scale = max(1.0, float(np.abs(b2).max()))
    assert np.all(np.abs(A @ x - b2) <= 1e-9 * scale)
    assert np.all(x >= lo2 - 1e-9) and np.all(x <= hi2 + 1e-9)
    assert g["obj"] == float(sum(float(c2[j] * x[j]) for j in range(len(x))))
    dual, primal, flips = g["iters"]
    assert dual == 0 or (primal == 0 and flips == 0)
    if pert == "cost":
        assert dual == 0   # the basis stays primal feasible


def test_cold_starts_exist():
    for kind in ("mixed", "box"):
        assert sum(_cold(s, kind)[6]["status"] == OPTIMAL for s in range(96)) >= 90


def _same_as_resolve_ref(A, b2, c, basis, mx, n_orig):
    n = A.shape[1]
    q = resolve_ref.resolve(A, b2, c, basis, mx, n_orig)
    g = W.resolve(A, b2, c, np.zeros(n), np.full(n, np.inf), basis, np.zeros(n, np.int32), mx, n_orig)
    assert g["status"] == q["status"]
    assert np.array_equal(g["basis"], q["basis"])
    assert tuple(g["iters"][:2]) == q["iters"] and g["iters"][2] == 0
    assert not g["at_upper"].any()
    if q["status"] == OPTIMAL:
        assert np.array_equal(g["x"], q["x"]) and g["obj"] == q["obj"]
    return q


@pytest.mark.parametrize("maximize", [True, False])
def test_identity_anchor_equals_resolve_ref(maximize):
    dual_runs = 0
    for seed in range(60):
        A, b2, c, basis, mx = _rhs_changed(seed, maximize=maximize)
        q = _same_as_resolve_ref(A, b2, c, basis, mx, A.shape[1] - A.shape[0])
        dual_runs += q["iters"][0] > 0
    assert dual_runs >= 40
    for seed in range(30):
        A, b2, c, basis, mx = _rhs_changed(seed, infeasible=True, maximize=maximize)
        assert _same_as_resolve_ref(A, b2, c, basis, mx, A.shape[1])["status"] == INFEASIBLE


def test_identity_anchor_other_outcomes():
    A, b2, c, basis, mx = _rhs_changed(4)
    c_bad = c.copy()
    c_bad[[j for j in range(A.shape[1]) if j not in set(basis.tolist())][0]] += 1e3
    assert _same_as_resolve_ref(A, b2, c_bad, basis, mx, A.shape[1])["status"] == BAD_ARG
    rep = basis.copy()
    rep[1] = rep[0]
    assert _same_as_resolve_ref(A, b2, c, rep, mx, A.shape[1])["status"] == SINGULAR
    slack = np.arange(A.shape[1] - A.shape[0], A.shape[1], dtype=np.int32)   # the crash is skipped
    assert _same_as_resolve_ref(A, b2, c, slack, mx, A.shape[1])["iters"][1] > 0


def test_cold_optimum_fed_back_unchanged():
    untouched = 0
    for s in range(96):
        A, b, c, lo, hi, mx, r = _cold(s, "mixed")
        if r["status"] != OPTIMAL:
            continue
        g = W.resolve(A, b, c, lo, hi, r["basis"], r["at_upper"], mx)
        assert g["status"] == OPTIMAL, s
        assert abs(g["obj"] - r["obj"]) <= 1e-9 * max(1.0, abs(r["obj"])), s
        untouched += g["iters"] == [0, 0, 0]
    assert untouched >= 90


def test_every_outcome_is_reached():
    max_iter = 3
    cases = W.outcome_cases(max_iter=max_iter)
    assert [name for name, _, _ in cases] == ["dual_complement", "primal_flip", "dual_infeasible", "crossed",
                                              "unbounded", "iter_limit", "singular", "no_valid_start"]
    for name, cs, status in cases:
        A, b, c, lo, hi, basis, up = cs
        g = W.resolve(*cs, True, max_iter=max_iter)
        assert g["status"] == status, name
        if status != OPTIMAL:
            assert np.isnan(g["obj"]) and np.all(np.isnan(g["x"])), name
        if name in ("crossed", "singular", "no_valid_start"):
            assert np.array_equal(g["basis"], basis) and np.array_equal(g["at_upper"], up), name
            assert g["iters"] == [0, 0, 0], name
        if name == "dual_complement":
            assert g["iters"][0] > 0 and g["iters"][1:] == [0, 0] and np.any(g["at_upper"] != up)
            st, z = _highs(A, b, c, lo, hi, True)
            assert st == OPTIMAL and abs(g["obj"] - z) <= 1e-7 * max(1.0, abs(z))
        if name == "primal_flip":
            assert g["iters"][0] == 0 and g["iters"][2] > 0
        if name == "dual_infeasible":
            assert not np.any(hi < lo) and g["iters"][0] >= 0 and _highs(A, b, c, lo, hi, True)[0] == INFEASIBLE
        if name == "crossed":
            assert np.any(hi < lo)
        if name == "iter_limit":
            assert g["iters"] == [max_iter, 0, 0]
            assert W.resolve(*cs, True, max_iter=0)["status"] == ITER_LIMIT


def test_reference_refuses_bad_starts():
    A, b, c, lo, hi, mx = B.boxed_lp(1, 6, 16)
    r = B.bounded(A, b, c, lo, hi, mx)
    assert r["status"] == OPTIMAL
    assert W.resolve(A, b, c, lo, hi, r["basis"], r["at_upper"], mx)["status"] == OPTIMAL
    free = int(np.flatnonzero(np.isinf(hi))[0])
    up = r["at_upper"].copy()
    up[free] = 1   # a flag on a column without an upper bound
    assert W.resolve(A, b, c, lo, hi, r["basis"], up, mx)["status"] == BAD_ARG
    up = r["at_upper"].copy()
    up[0] = 2
    assert W.resolve(A, b, c, lo, hi, r["basis"], up, mx)["status"] == BAD_ARG
    for bad in (-1, 16):
        basis = r["basis"].copy()
        basis[2] = bad
        assert W.resolve(A, b, c, lo, hi, basis, r["at_upper"], mx)["status"] == BAD_ARG
    for j, (l, h) in enumerate(((-np.inf, 1.0), (np.nan, 1.0), (0.0, np.nan))):
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[j], hi2[j] = l, h
        assert W.resolve(A, b, c, lo2, hi2, r["basis"], np.zeros(16, np.int32), mx)["status"] == BAD_ARG


def test_capi_refuses_without_a_context():
    lib = capi.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    z = np.zeros(16)
    zi = np.zeros(16, np.int32)
    d, i = z.ctypes.data_as(dp), zi.ctypes.data_as(ip)
    assert lib.lp_simplex_bounded_resolve(None, d, 2, 4, d, d, d, d, i, i, 1, 4, 1e-9, 10, d, i, i, d, i) == BAD_ARG
    assert lib.lp_simplex_bounded_resolve_batched(None, 1, d, 2, 4, d, d, d, d, i, i, 1, 4, 1e-9, 10, d, i, i, d, i,
                                                  i) == BAD_ARG
