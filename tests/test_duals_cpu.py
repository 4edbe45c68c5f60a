"""CPU-only checks of the dual solution at a basis: the test restatement (tests/ref/duals_ref.c) solves
B^T y = c_B, certifies the oracle's optima by strong duality, dual feasibility and complementary slackness,
matches HiGHS's shadow prices on the golden cases, and the C ABI refuses null arguments without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import duals_ref as D
from tests import lpcases

HERE = os.path.dirname(os.path.abspath(__file__))


def _lp(seed):
    """(A, b, c, starting basis, maximize): slack-basis max LPs, non-slack-basis general LPs of both senses."""
    m = 2 + seed % 17
    if seed % 2:
        A, b, c, basis = lpcases.general_lp(seed, m, 2 * m + seed % 5)
        return A, b, c, basis, bool(seed % 4 == 1)
    A, b, c, basis = capi.gen_lp(seed, m, 2 * m + 3 + seed % 7)
    return A, b, c, basis, True


@pytest.mark.parametrize("seed", range(30))
def test_solves_the_transposed_basis_system(seed):
    A, b, c, basis, _ = _lp(seed)
    r = D.duals(A, b, c, basis)
    assert r["status"] == o.OPTIMAL
    y = np.linalg.solve(A[:, basis].T, c[basis])
    assert np.allclose(r["y"], y, rtol=1e-12, atol=1e-12 * np.abs(y).max())
    d = c - A.T @ r["y"]
    d[basis] = 0.0
    assert np.allclose(r["d"], d, rtol=0, atol=1e-12 * (1 + np.abs(c).max()))
    assert np.array_equal(r["d"][basis], np.zeros(len(basis)))
    assert r["w"] == pytest.approx(float(b @ r["y"]), rel=1e-12, abs=1e-12)


@pytest.mark.parametrize("seed", range(30))
def test_certifies_the_oracle_optimum(seed):
    A, b, c, basis, mx = _lp(seed)
    q = o.simplex_tableau(A, b, c, basis, mx, A.shape[1])
    if q["status"] != o.OPTIMAL:
        return   # (general_lp min problems can be unbounded: nothing to certify)
    r = D.duals(A, b, c, q["basis"])
    assert r["status"] == o.OPTIMAL
    z = q["obj"]
    assert abs(r["w"] - z) <= 1e-9 * (1 + abs(z))                  # strong duality
    if mx:
        assert r["d"].max() <= 1e-9                                # dual feasibility, max
    else:
        assert r["d"].min() >= -1e-9                               # dual feasibility, min
    assert np.array_equal(r["d"][q["basis"]], np.zeros(A.shape[0]))
    assert abs(float(r["d"] @ q["x"])) <= 1e-9 * (1 + abs(z))      # complementary slackness


def test_certifies_two_phase_optima_of_min_problems():
    for seed in range(20):
        A, b, c, no = lpcases.min_lp(seed, 3 + seed % 9, 4 + seed % 11, equalities=seed % 2,
                                     negative_rows=seed % 3)
        q = o.two_phase(A, b, c, False, A.shape[1])
        assert q["status"] == o.OPTIMAL
        r = D.duals(A, b, c, q["basis"])
        assert r["status"] == o.OPTIMAL
        assert abs(r["w"] - q["obj"]) <= 1e-9 * (1 + abs(q["obj"]))
        assert r["d"].min() >= -1e-9


def test_golden_highs_marginals():
    cases = json.load(open(os.path.join(HERE, "golden", "dual_cases.json")))
    assert len(cases) >= 12 and {g["maximize"] for g in cases} == {True, False}
    for g in cases:
        if g["kind"] == "gen_lp":
            A, b, c, _ = capi.gen_lp(*g["args"])
        else:
            A, b, c, _ = lpcases.min_lp(*g["args"])
        r = D.duals(A, b, c, np.array(g["basis"], np.int32))
        assert r["status"] == o.OPTIMAL
        y = np.array(g["y"])
        assert np.allclose(r["y"], y, rtol=0, atol=1e-9 * (1 + np.abs(y).max())), g["args"]
        assert abs(r["w"] - g["obj"]) <= 1e-9 * (1 + abs(g["obj"]))


def test_singular_and_out_of_range_bases():
    A, b, c, basis = capi.gen_lp(3, 6, 14)
    Bs = basis.copy()
    Bs[2] = Bs[0]   # repeated column
    r = D.duals(A, b, c, Bs)
    assert r["status"] == o.SINGULAR and np.isnan(r["y"]).all() and np.isnan(r["d"]).all() and np.isnan(r["w"])
    A2 = A.copy()
    A2[:, 1] = A2[:, 0] * (1 + 1e-15)   # numerically dependent columns
    r = D.duals(A2, b, c, np.array([0, 1, 2, 3, 4, 5], np.int32))
    assert r["status"] == o.SINGULAR
    Bo = basis.copy()
    Bo[1] = A.shape[1]
    assert D.duals(A, b, c, Bo)["status"] == o.BAD_ARG
    Bo[1] = -1
    assert D.duals(A, b, c, Bo)["status"] == o.BAD_ARG


def test_slack_identity_needs_no_crash():
    """At the slack identity the crash is exact: y = c_B bit for bit."""
    A, b, c, basis = capi.gen_lp(5, 9, 20)
    c = c.copy()
    c[basis] = np.linspace(-1, 1, len(basis))
    r = D.duals(A, b, c, basis)
    assert np.array_equal(r["y"], c[basis])


def test_abi_rejects_null_arguments_without_a_device():
    lib = capi.load()
    m, n, batch = 2, 4, 2
    A = np.zeros(batch * m * n)
    b, c = np.ones(batch * m), np.ones(batch * n)
    basis = np.zeros(batch * m, np.int32)
    y, d, w = np.zeros(batch * m), np.zeros(batch * n), np.zeros(batch)
    st = np.zeros(batch, np.int32)
    dp, ip = capi._d, capi._i
    assert lib.lp_basis_duals(None, dp(A), m, n, dp(b), dp(c), ip(basis), dp(y), dp(d), dp(w)) == capi.BAD_ARG
    assert lib.lp_basis_duals_batched(None, batch, dp(A), m, n, dp(b), dp(c), ip(basis), dp(y), dp(d), dp(w),
                                      ip(st)) == capi.BAD_ARG
    assert lib.lp_batched_duals(None, dp(y), dp(d), dp(w), ip(st)) == capi.BAD_ARG
    assert lib.lp_basis_duals_fits(64) == 1 and lib.lp_basis_duals_fits(128) == 1
    assert lib.lp_basis_duals_fits(140) == 1 and lib.lp_basis_duals_fits(512) == 0
    assert lib.lp_basis_duals_fits(0) == 0
    # every shape the batched two-phase and re-solve kernels run fits
    for m in range(1, 141):
        assert lib.lp_basis_duals_fits(m) == 1
