"""Farkas and unbounded-ray certificates of bounded-variable LPs: tests/ref/bounded_certificate_ref.c alone, on the
CPU.  Every FARKAS vector and every RAY is checked with numpy against the box, independently of the definition's chains;
the bases and flags come from the bounded two-phase and re-solve references.  Also: the anchor on
tests/ref/certificate_ref.c, the refusals, and the kernel's LDS carve against lp_basis_bounded_certificate_fits (a host
call)."""
import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import bounded_certcases as BC
from tests import bounded_certificate_ref as R
from tests import certcases as CC
from tests import certificate_ref as CR
from tests import resolve_ref as RS

NONE, FARKAS, RAY = R.NONE, R.FARKAS, R.RAY


def cert_of(cs, eps=1e-9):
    return R.certificate(cs["A"], cs["b"], cs["c"], cs["lo"], cs["hi"], cs["basis"], cs["at_upper"], cs["maximize"],
                         eps)


@pytest.mark.parametrize("m,n", BC.SHAPES)
def test_infeasible_gets_farkas_from_phase_one(m, n):
    for seed in BC.SEEDS:
        cs = BC.cold(seed, m, n, "infeasible")
        assert cs["run"] == R.INFEASIBLE and (cs["basis"] >= n).any()
        cert = cert_of(cs)
        assert cert["status"] == R.OPTIMAL and cert["kind"] == FARKAS and cert["index"] == -1, seed
        BC.check(cs, cert)


@pytest.mark.parametrize("m,n", BC.SHAPES)
def test_unbounded_gets_ray(m, n):
    for seed in BC.SEEDS:
        cs = BC.cold(seed, m, n, "unbounded")
        assert cs["run"] == R.UNBOUNDED
        cert = cert_of(cs)
        assert cert["status"] == R.OPTIMAL and cert["kind"] == RAY, seed
        BC.check(cs, cert)


@pytest.mark.parametrize("m,n", BC.SHAPES)
def test_rich_unbounded_ray_moves_the_basis(m, n):
    for seed in BC.SEEDS:
        cs = BC.rich_unbounded(seed, m, n)
        assert cs["run"] == R.UNBOUNDED
        cert = cert_of(cs)
        assert cert["status"] == R.OPTIMAL and cert["kind"] == RAY, seed
        BC.check(cs, cert)
        assert np.count_nonzero(cert["ray"]) > 1, seed


@pytest.mark.parametrize("m,n", BC.SHAPES)
def test_crossed_is_infeasible_without_a_vector(m, n):
    for seed in BC.SEEDS:
        cs = BC.cold(seed, m, n, "crossed")
        assert cs["run"] == R.INFEASIBLE
        cert = cert_of(cs)
        assert cert["status"] == R.INFEASIBLE, seed
        BC.check(cs, cert)
        assert cert["kind"] == NONE


@pytest.mark.parametrize("m,n", BC.SHAPES)
def test_mixed_optimum_has_no_certificate(m, n):
    optimal = 0
    for seed in BC.SEEDS:
        cs = BC.cold(seed, m, n, "mixed")
        cert = cert_of(cs)
        assert cert["status"] == R.OPTIMAL
        BC.check(cs, cert)
        if cs["run"] == R.OPTIMAL:
            optimal += 1
            assert cert["kind"] == NONE, seed
        elif cs["run"] == R.INFEASIBLE:
            assert cert["kind"] == FARKAS, seed
        elif cs["run"] == R.UNBOUNDED:
            assert cert["kind"] == RAY, seed
    assert optimal >= len(BC.SEEDS) // 2


def test_dual_infeasible_gets_farkas_from_a_violated_row():
    """Every re-solve a tightened bound drives to INFEASIBLE gets FARKAS from the dual case, and both sides occur: a
    basic variable below its lower bound and one above its upper bound."""
    total, below, above = 0, 0, 0
    for m, n in BC.SHAPES:
        for seed in BC.SEEDS:
            cs = BC.dual_infeasible(seed, m, n)
            if cs is None:
                continue
            total += 1
            assert (cs["basis"] < n).all()
            cert = cert_of(cs)
            assert cert["status"] == R.OPTIMAL and cert["kind"] == FARKAS and 0 <= cert["index"] < m, (m, n, seed)
            BC.check(cs, cert)
            # which bound the certified position violates, from numpy's own xB
            k = cs["basis"][cert["index"]]
            Bm = cs["A"][:, cs["basis"]]
            v = np.where(cs["at_upper"] == 1, cs["hi"], cs["lo"])
            v[cs["basis"]] = 0.0
            xk = np.linalg.solve(Bm, cs["b"] - cs["A"] @ v)[cert["index"]]
            if xk < cs["lo"][k]:
                below += 1
                assert abs(cert["value"] - (xk - cs["lo"][k])) <= 1e-8
            else:
                assert xk > cs["hi"][k]
                above += 1
                assert abs(cert["value"] - (cs["hi"][k] - xk)) <= 1e-8
    assert total >= 20 and below >= 1 and above >= 1, (total, below, above)


def test_certificate_at_the_eps_boundary_is_none():
    """One row x0 + s = 1 with x0 fixed at 2 and s in [0, inf): infeasible by 1.  eps above the violation: NONE."""
    A, b, c = np.array([[1.0, 1.0]]), np.array([1.0]), np.array([1.0, 0.0])
    lo, hi = np.array([2.0, 0.0]), np.array([2.0, np.inf])
    for basis, up in (([2], [0, 0]), ([1], [0, 0])):   # phase I; s basic below its lower bound
        r = R.certificate(A, b, c, lo, hi, basis, up, True)
        assert r["status"] == R.OPTIMAL and r["kind"] == FARKAS and r["value"] == -1.0, basis
        BC.check(dict(A=A, b=b, c=c, lo=lo, hi=hi, maximize=True), r)
        r = R.certificate(A, b, c, lo, hi, basis, up, True, eps=1.5)
        assert r["status"] == R.OPTIMAL and r["kind"] == NONE and np.isnan(r["value"]) and r["index"] == -1
    # a fixed column is tested by its flag: held "at hi" its weight +1 fails g <= eps, and the answer is NONE
    r = R.certificate(A, b, c, lo, hi, [1], [1, 0], True)
    assert r["status"] == R.OPTIMAL and r["kind"] == NONE
    # above an upper bound: x0 in [0, 0.25] basic at 0.5 with s held at its upper bound 0.5
    lo, hi = np.array([0.0, 0.0]), np.array([0.25, 0.5])
    r = R.certificate(A, b, c, lo, hi, [0], [0, 1], True)
    assert r["kind"] == FARKAS and r["index"] == 0 and r["farkas"][0] == -1.0 and r["value"] == -0.25
    assert R.certificate(A, b, c, lo, hi, [0], [0, 0], True)["kind"] == NONE   # s at 0: x0 = 1, but s can still grow
    BC.check(dict(A=A, b=b, c=c, lo=lo, hi=hi, maximize=True), r)


def _same_as_unbounded_reference(A, b, c, basis, maximize):
    m, n = A.shape
    want = CR.certificate(A, b, c, basis, maximize)
    got = R.certificate(A, b, c, np.zeros(n), np.full(n, np.inf), basis, np.zeros(n, np.int32), maximize)
    R.same_bits(got, want)
    return want["kind"]


def test_anchor_two_phase_mix():
    kinds = set()
    for m, k in [(6, 9), (10, 16), (24, 40)]:
        A, b, c, _ = CC.two_phase_mix(100 * m, 16, m, k)
        for q in range(len(A)):
            r = o.two_phase(A[q], b[q], c[q], False)
            kinds.add(_same_as_unbounded_reference(A[q], b[q], c[q], r["basis"], False))
    assert kinds == {NONE, FARKAS, RAY}


def test_anchor_plain_mix():
    kinds = set()
    for m, n in [(6, 14), (12, 30), (32, 64)]:
        A, b, c, basis, _ = CC.plain_mix(10 * m, 12, m, n)
        for q in range(len(A)):
            r = o.simplex_tableau(A[q], b[q], c[q], basis[q], True)
            kinds.add(_same_as_unbounded_reference(A[q], b[q], c[q], r["basis"], True))
            _same_as_unbounded_reference(A[q], b[q], c[q], basis[q], True)
    assert kinds == {NONE, RAY}


def test_anchor_resolve_mix():
    kinds = set()
    for m, n in [(6, 14), (16, 40)]:
        A, b, b2, c, basis, _ = CC.resolve_mix(7 * m, 10, m, n)
        for q in range(len(A)):
            s = o.simplex_tableau(A[q], b[q], c[q], basis[q], True)
            r = RS.resolve(A[q], b2[q], c[q], s["basis"], True)
            kinds.add(_same_as_unbounded_reference(A[q], b2[q], c[q], r["basis"], True))
    assert kinds == {NONE, FARKAS}


def test_refusals():
    A, b, c, lo, hi, mx = BC.B.boxed_lp(3, 4, 12, kind="mixed")
    m, n = A.shape
    r0 = BC.B.bounded(A, b, c, lo, hi, mx)
    basis, up = r0["basis"], r0["at_upper"]
    free = int(np.flatnonzero(np.isinf(hi))[0])

    def run(lo=lo, hi=hi, basis=basis, up=up, eps=1e-9):
        r = R.certificate(A, b, c, lo, hi, basis, up, mx, eps)
        assert r["kind"] == NONE and np.isnan(r["farkas"]).all() and np.isnan(r["ray"]).all()
        assert np.isnan(r["value"]) and r["index"] == -1
        return r["status"]

    def with_(v, j, x):
        v = np.array(v, dtype=np.float64 if np.asarray(v).dtype.kind == "f" else np.int32)
        v[j] = x
        return v

    assert run(eps=-1.0) == R.BAD_ARG and run(eps=float("nan")) == R.BAD_ARG
    assert run(lo=with_(lo, 1, np.nan)) == R.BAD_ARG and run(lo=with_(lo, 1, -np.inf)) == R.BAD_ARG
    assert run(hi=with_(hi, 1, np.nan)) == R.BAD_ARG
    assert run(up=with_(up, 2, 2)) == R.BAD_ARG and run(up=with_(up, 2, -1)) == R.BAD_ARG
    assert run(up=with_(up, free, 1)) == R.BAD_ARG                       # a flag on an infinite hi
    assert run(basis=with_(basis, 0, n + m)) == R.BAD_ARG and run(basis=with_(basis, 0, -1)) == R.BAD_ARG
    assert run(basis=with_(basis, 1, basis[0])) == R.SINGULAR            # a repeated column
    assert run(basis=np.array([n, 1, 2, n])) == R.SINGULAR               # a repeated artificial
    assert run(hi=with_(hi, 1, lo[1] - 0.5)) == R.INFEASIBLE             # crossed bounds
    assert run(hi=with_(hi, 1, -np.inf)) == R.INFEASIBLE
    assert run(hi=with_(hi, 1, lo[1] - 0.5), basis=with_(basis, 1, basis[0])) == R.INFEASIBLE   # crossed comes first
    A2 = A.copy()
    A2[:, 1] = 2.0 * A2[:, 0]
    r = R.certificate(A2, b, c, np.zeros(n), np.full(n, np.inf), [0, 1, 2, 3], np.zeros(n, np.int32), mx)
    assert r["status"] == R.SINGULAR and r["kind"] == NONE               # dependent columns
    assert R.certificate(A, b, c, lo, hi, np.arange(n, n + m), np.zeros(n, np.int32), mx)["status"] == R.OPTIMAL


def carve_bytes(m, n):
    """The LDS carve of k_batched_bounded_certificate, restated: doubles pub (2), T (m x pitch, pitch odd), the scratch
    region (the 256 x 9 A tile or lcol + prow), f, b', L, H (m each), v (n); ints rowpos, used, zneg, slot (m each), pos
    (n), okr (8)."""
    pitch = (m + 1) | 1
    scratch = max(256 * 9, 2 * m + 1)
    return 8 * (2 + m * pitch + scratch + 4 * m + n) + 4 * (4 * m + n + 8)


def test_fits_is_the_bounded_fit_and_the_carve():
    lib = capi.load()
    fits = lib.lp_basis_bounded_certificate_fits
    assert fits(64, 192) == 1 and carve_bytes(64, 192) <= 160 * 1024
    assert fits(0, 4) == 0 and fits(4, 3) == 0 and fits(-1, -1) == 0
    carve_only = []   # shapes the bounded simplex takes and the certificate's carve does not
    for m in list(range(1, 150)) + [180, 200]:
        for n in (m, m + 1, m + 7, 2 * m, 3 * m, 8 * m, 40 * m):
            bounded = lib.lp_simplex_bounded_fits(m, n) == 1
            carve = carve_bytes(m, n) <= 160 * 1024
            assert fits(m, n) == int(bounded and carve), (m, n)
            if bounded and not carve:
                carve_only.append((m, n))
    assert carve_only, "no shape on the far side of the carve's limit"
    # both sides of the carve's limit at n = m
    m = min(mm for mm, nn in carve_only if nn == mm)
    assert carve_bytes(m - 1, m - 1) <= 160 * 1024 < carve_bytes(m, m)
    assert fits(m - 1, m - 1) == 1 and fits(m, m) == 0 and lib.lp_simplex_bounded_fits(m, m) == 1
