"""Farkas and unbounded-ray certificates: tests/ref/certificate_ref.c alone, on the CPU.  Every FARKAS vector and
every RAY is checked with numpy, HiGHS agrees with the verdict, and an optimal basis has no certificate.  The bases
come from the oracle's two-phase and tableau simplex and from the re-solve reference."""
import numpy as np
import pytest
from scipy.optimize import linprog

from oracle import pyoracle as o
from tests import certcases as CC
from tests import certificate_ref as R
from tests import ranging_ref as RR
from tests import resolve_ref as RS

NONE, FARKAS, RAY = 0, 1, 2
TOL = 1e-7


def check_farkas(A, b, f):
    assert np.all(np.isfinite(f))
    assert (A.T @ f >= -TOL * max(1.0, np.abs(f).max())).all()
    assert b @ f < 0


def check_ray(A, c, r, maximize):
    assert np.all(np.isfinite(r))
    assert np.linalg.norm(A @ r) <= TOL * max(1.0, np.abs(A).max() * np.abs(r).max())
    assert (r >= -TOL).all()
    assert (c @ r > 0) if maximize else (c @ r < 0)


def check(A, b, c, maximize, cert):
    """The certificate's own properties and the NaN layout of its kind."""
    assert cert["status"] == 0
    if cert["kind"] == FARKAS:
        check_farkas(A, b, cert["farkas"])
        assert np.isnan(cert["ray"]).all()
        assert cert["value"] < 0
    elif cert["kind"] == RAY:
        check_ray(A, c, cert["ray"], maximize)
        assert np.isnan(cert["farkas"]).all()
        assert cert["ray"][cert["index"]] == 1.0
    else:
        assert np.isnan(cert["farkas"]).all() and np.isnan(cert["ray"]).all() and np.isnan(cert["value"])
        assert cert["index"] == -1


def highs_status(A, b, c, maximize):
    return linprog(-c if maximize else c, A_eq=A, b_eq=b, bounds=(0, None), method="highs").status


@pytest.mark.parametrize("m,k", [(6, 9), (10, 16), (24, 40)])
def test_two_phase_families(m, k):
    A, b, c, names = CC.two_phase_mix(100 * m, 16, m, k)
    for q, fam in enumerate(names):
        r = o.two_phase(A[q], b[q], c[q], False)
        cert = R.certificate(A[q], b[q], c[q], r["basis"], False)
        check(A[q], b[q], c[q], False, cert)
        hs = highs_status(A[q], b[q], c[q], False)
        if fam == "optimal":
            assert r["status"] == 0 and hs == 0 and cert["kind"] == NONE
        elif fam == "phase2_unbounded":
            assert r["status"] == 1 and hs == 3 and cert["kind"] == RAY
        else:
            assert r["status"] == 4 and hs == 2 and cert["kind"] == FARKAS and cert["index"] == -1
            assert (r["basis"] >= A.shape[2]).any()   # the phase-I case
            if fam == "infeasible_rows":
                assert np.count_nonzero(cert["farkas"]) > 1


@pytest.mark.parametrize("m,n", [(6, 14), (12, 30), (32, 64)])
def test_plain_families(m, n):
    A, b, c, basis, names = CC.plain_mix(10 * m, 12, m, n)
    for q, fam in enumerate(names):
        r = o.simplex_tableau(A[q], b[q], c[q], basis[q], True)
        cert = R.certificate(A[q], b[q], c[q], r["basis"], True)
        check(A[q], b[q], c[q], True, cert)
        hs = highs_status(A[q], b[q], c[q], True)
        at_start = R.certificate(A[q], b[q], c[q], basis[q], True)
        if fam == "optimal":
            assert r["status"] == 0 and hs == 0 and cert["kind"] == NONE
        else:
            assert r["status"] == 1 and hs == 3 and cert["kind"] == RAY
            assert at_start["kind"] == (RAY if fam == "unbounded_obvious" else NONE)
            if fam == "unbounded_after_pivots":
                assert r["iters"] >= 1


@pytest.mark.parametrize("m,n", [(6, 14), (16, 40)])
def test_resolve_family(m, n):
    A, b, b2, c, basis, names = CC.resolve_mix(7 * m, 10, m, n)
    for q, fam in enumerate(names):
        s = o.simplex_tableau(A[q], b[q], c[q], basis[q], True)
        r = RS.resolve(A[q], b2[q], c[q], s["basis"], True)
        cert = R.certificate(A[q], b2[q], c[q], r["basis"], True)
        check(A[q], b2[q], c[q], True, cert)
        if fam == "optimal":
            assert r["status"] == 0 and cert["kind"] == NONE
        else:
            assert r["status"] == 4 and highs_status(A[q], b2[q], c[q], True) == 2
            assert cert["kind"] == FARKAS and 0 <= cert["index"] < m
            assert r["iters"][0] >= 1   # the dual simplex ran


@pytest.mark.parametrize("maximize", [True, False])
def test_optimal_bases_have_no_certificate(maximize):
    for seed in range(8):
        A, b, c, basis = CC.capi.gen_lp(seed, 8, 20)
        if not maximize:
            c = -c
        r = o.simplex_tableau(A, b, c, basis, maximize)
        assert r["status"] == 0
        cert = R.certificate(A, b, c, r["basis"], maximize)
        check(A, b, c, maximize, cert)
        assert cert["kind"] == NONE


def test_crash_matches_ranging_without_artificials():
    for seed in range(6):
        A, b, c, basis = CC.capi.gen_lp(seed, 9, 21)
        r = o.simplex_tableau(A, b, c, basis, True)
        st, binv, xb = R.crash(A, b, r["basis"])
        st2, binv2, xb2 = RR.crash(A, b, r["basis"], False)
        assert st == st2 == 0
        assert np.array_equal(binv.view(np.uint64), binv2.view(np.uint64))
        assert np.array_equal(xb.view(np.uint64), xb2.view(np.uint64))


def test_artificial_column_sign():
    """Artificial n+i is s_i e_i with s_i = -1 for b_i < -eps: one row, x >= 0, x = -1 is infeasible, and the
    artificial basis gives xB = 1 (the flipped row's value) and f = +1."""
    A, b, c = np.array([[1.0, 2.0]]), np.array([-1.0]), np.array([1.0, 1.0])
    st, binv, xb = R.crash(A, b, [2])
    assert st == 0 and binv[0, 0] == -1.0 and xb[0] == 1.0
    cert = R.certificate(A, b, c, [2], False)
    assert cert["kind"] == FARKAS and cert["farkas"][0] == 1.0 and cert["value"] == -1.0
    # at the eps boundary: an artificial sum <= eps gives NONE
    cert = R.certificate(A, np.array([-1e-12]), c, [2], False, eps=1e-9)
    assert cert["status"] == 0 and cert["kind"] == NONE


def test_bad_arg_and_singular():
    A, b, c, basis = CC.capi.gen_lp(3, 4, 10)
    m, n = A.shape
    for bad in ([0, 1, 2, n + m], [-1, 1, 2, 3]):
        r = R.certificate(A, b, c, bad)
        assert r["status"] == 5 and r["kind"] == NONE and np.isnan(r["farkas"]).all() and np.isnan(r["ray"]).all()
    assert R.certificate(A, b, c, basis, eps=-1.0)["status"] == 5
    assert R.certificate(A, b, c, basis, eps=float("nan"))["status"] == 5
    assert R.certificate(A, b, c, [n, 1, 2, n])["status"] == 3        # a repeated artificial
    assert R.certificate(A, b, c, [0, 1, 1, 3])["status"] == 3        # a repeated column
    A2 = A.copy()
    A2[:, 1] = 2.0 * A2[:, 0]
    r = R.certificate(A2, b, c, [0, 1, 2, 3])
    assert r["status"] == 3 and r["kind"] == NONE and r["index"] == -1   # dependent columns
    assert R.certificate(A, b, c, [n + 0, n + 1, n + 2, n + 3])["status"] == 0   # all artificials
