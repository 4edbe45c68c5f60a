"""CPU-only checks of the re-solve from a given basis: the test restatement (tests/ref/resolve_ref.c) equals
the oracle's tableau simplex bit for bit on its primal branch, its dual branch reaches the optimum of a
cold two-phase solve of the changed LP, and the C ABI refuses null arguments without a device."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import lpcases
from tests import resolve_ref as R


def _optimal_basis(A, b, c, basis, maximize=True):
    q = o.simplex_tableau(A, b, c, basis, maximize, A.shape[1])
    assert q["status"] == o.OPTIMAL
    return q["basis"]


def _cost_changed(seed):
    """(A, b, c', optimal basis of (A, b, c), maximize, n_orig): only the costs changed, so the old basis
    stays primal feasible."""
    rng = np.random.default_rng(300 + seed)
    m = 2 + seed % 13
    n = 2 * m + seed % 4
    if seed % 3 == 0:
        A, b, c, basis = lpcases.general_lp(seed, m, n)
        mx, no = bool(seed % 2), A.shape[1]
    else:
        A, b, c, basis = lpcases.random_lp(seed, m, n)
        mx, no = True, n - m
    B = _optimal_basis(A, b, c, basis, mx)
    c2 = c * rng.uniform(0.5, 1.5, size=c.shape) + rng.uniform(-0.2, 0.2, size=c.shape) * (c != 0)
    return A, b, c2, B, mx, no


@pytest.mark.parametrize("seed", range(40))
def test_primal_branch_is_the_oracle(seed):
    A, b, c2, B, mx, no = _cost_changed(seed)
    r = R.resolve(A, b, c2, B, mx, no, trace_cap=1 << 14, want_tableau=True)
    q = o.simplex_tableau(A, b, c2, B, mx, no, trace_cap=1 << 14, want_tableau=True)
    assert r["status"] == q["status"]
    assert r["iters"] == (0, q["iters"])
    assert r["trace"] == q["trace"]
    assert np.array_equal(r["basis"], q["basis"])
    assert np.array_equal(r["tableau"], q["tableau"])
    if q["status"] == o.OPTIMAL:
        assert np.array_equal(r["x"], q["x"]) and r["obj"] == q["obj"]


def test_primal_branch_from_the_slack_basis():
    """The slack identity with zero costs skips the crash, as in the oracle."""
    for seed in range(10):
        A, b, c, basis = lpcases.random_lp(seed, 6 + seed, 16 + 2 * seed)
        no = A.shape[1] - A.shape[0]
        r = R.resolve(A, b, c, basis, True, no, trace_cap=1 << 12, want_tableau=True)
        q = o.simplex_tableau(A, b, c, basis, True, no, trace_cap=1 << 12, want_tableau=True)
        assert (r["status"], r["iters"], r["trace"]) == (q["status"], (0, q["iters"]), q["trace"])
        assert np.array_equal(r["tableau"], q["tableau"])


def _rhs_changed(seed, infeasible=False, maximize=True):
    """gen_lp, its optimal basis, and b' with 1-4 rows scaled down (or one row set far below 0 when
    `infeasible`: every coefficient of a gen_lp row is >= 0, so the row has no solution)."""
    m = 3 + seed % 20
    n = m + 4 + (seed * 7) % 30
    A, b, c, basis = lpcases.random_lp(seed, m, n)
    B = _optimal_basis(A, b, c, basis)
    b2 = R.scale_rows(seed, b)
    if infeasible:
        b2[seed % m] = -(1.0 + 0.01 * seed) * (n - m)
    return A, b2, (c if maximize else -c), B, maximize


@pytest.mark.parametrize("maximize", [True, False])
def test_dual_branch_reaches_the_cold_optimum(maximize):
    dual_runs = 0
    for seed in range(60):
        A, b2, c, B, mx = _rhs_changed(seed, maximize=maximize)
        n = A.shape[1]
        r = R.resolve(A, b2, c, B, mx, n)
        q = o.two_phase(A, b2, c, mx, n)
        assert r["status"] == q["status"] == o.OPTIMAL, seed
        z = q["obj"]
        assert abs(r["obj"] - z) <= 1e-9 * max(1.0, abs(z)), seed
        assert np.all(r["x"] >= -1e-9)
        assert np.allclose(A @ r["x"], b2, rtol=0, atol=1e-8 * max(1.0, np.abs(b2).max()))
        dual, primal = r["iters"]
        assert primal == 0 or dual == 0
        dual_runs += dual > 0
    assert dual_runs >= 40   # most of the perturbed bases are primal infeasible


def test_dual_branch_detects_infeasibility():
    for seed in range(30):
        A, b2, c, B, mx = _rhs_changed(seed, infeasible=True, maximize=bool(seed % 2))
        r = R.resolve(A, b2, c, B, mx)
        q = o.two_phase(A, b2, c, mx)
        assert r["status"] == q["status"] == o.INFEASIBLE, seed
        assert r["iters"][1] == 0 and r["iters"][0] >= 0


def test_neither_feasible_singular_and_iteration_limit():
    A, b2, c, B, mx = _rhs_changed(4)
    assert R.resolve(A, b2, c, B, mx)["status"] == o.OPTIMAL
    c_bad = c.copy()
    c_bad[[j for j in range(A.shape[1]) if j not in set(B.tolist())][0]] += 1e3   # breaks dual feasibility
    r = R.resolve(A, b2, c_bad, B, mx)
    assert r["status"] == o.BAD_ARG and np.array_equal(r["basis"], B) and r["iters"] == (0, 0)
    Bs = B.copy()
    Bs[1] = Bs[0]   # repeated column
    r = R.resolve(A, b2, c, Bs, mx)
    assert r["status"] == o.SINGULAR and np.array_equal(r["basis"], Bs)
    full = R.resolve(A, b2, c, B, mx, trace_cap=64)
    assert full["iters"][0] >= 2
    for k in (0, 1, 2):
        r = R.resolve(A, b2, c, B, mx, max_iter=k, trace_cap=64)
        assert r["status"] == o.ITER_LIMIT and r["iters"] == (k, 0)
        assert r["trace"] == full["trace"][:k]


def test_abi_rejects_null_arguments_without_a_device():
    lib = capi.load()
    m, n, batch = 2, 4, 2
    A = np.zeros(batch * m * n)
    b, c = np.ones(batch * m), np.ones(batch * n)
    basis = np.zeros(batch * m, np.int32)
    x, obj = np.zeros(batch * n), np.zeros(batch)
    bo, it, st = np.zeros(batch * m, np.int32), np.zeros(batch * 2, np.int32), np.zeros(batch, np.int32)
    d, i = capi._d, capi._i
    assert lib.lp_simplex_resolve(None, d(A), m, n, d(b), d(c), i(basis), 1, n, 1e-9, 100, d(x), i(bo), d(obj),
                                  i(it)) == capi.BAD_ARG
    assert lib.lp_simplex_resolve(None, d(A), 3, n, d(b), d(c), i(basis), 1, n, 1e-9, 100, d(x), i(bo), d(obj),
                                  i(it)) == capi.BAD_ARG
    assert lib.lp_simplex_resolve_batched(None, batch, d(A), m, n, d(b), d(c), i(basis), 1, n, 1e-9, 100, d(x),
                                          i(bo), d(obj), i(it), i(st)) == capi.BAD_ARG
    h = C.c_void_p()
    assert lib.lp_batched_resolve_upload(None, batch, d(A), m, n, d(b), d(c), i(basis), 1, n,
                                         C.byref(h)) == capi.BAD_ARG
    assert not h.value
    assert lib.lp_simplex_resolve_run(None, 1e-9, 100, i(it), None) == capi.BAD_ARG
    assert lib.lp_batched_set_start(None, d(b), i(basis)) == capi.BAD_ARG
    assert lib.lp_batched_resolve_iters(None, i(it)) == capi.BAD_ARG
