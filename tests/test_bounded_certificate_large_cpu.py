"""What the cases of tests/bounded_certificate_large_cases.py must show, asserted against the reference alone
(tests/ref/bounded_certificate_ref.c): tests/test_gpu_bounded_certificate_large.py compares the GPU with the reference on
exactly these cases, so a case that stopped exercising its branch would pass there unnoticed.  No GPU."""
import numpy as np
import pytest

from tests import bounded_certcases as BC
from tests import bounded_certificate_large_cases as L
from tests import bounded_certificate_ref as CR

EPS = 1e-9


def _artificials(cs):
    return int((np.asarray(cs["basis"]) >= cs["A"].shape[1]).sum())


def _xb(cs):
    """The basic values of a basis without artificials, by numpy."""
    A, b, lo, hi, basis, up = (cs[k] for k in ("A", "b", "lo", "hi", "basis", "at_upper"))
    v = np.where(np.asarray(up) == 1, hi, lo)
    v[basis] = 0.0
    return np.linalg.solve(A[:, basis], b - A @ v)


@pytest.mark.parametrize("key", L.COLD, ids=str)
def test_cold(key):
    cs = L.cold(*key)
    r = L.ref(("cold",) + key, cs)
    m, n = cs["A"].shape
    if key[0] == "infeasible":
        assert (cs["run"], r["status"], r["kind"], r["index"]) == (L.INFEASIBLE, L.OPTIMAL, L.FARKAS, -1)
        assert _artificials(cs) == m   # a signed identity: the s_i signs and little else
    elif key[0] == "unbounded":
        assert (cs["run"], r["status"], r["kind"]) == (L.UNBOUNDED, L.OPTIMAL, L.RAY)
        assert np.count_nonzero(r["ray"]) == 1
    else:
        assert (cs["run"], r["status"], r["kind"]) == (L.INFEASIBLE, L.INFEASIBLE, L.NONE)
    BC.check(cs, r)


@pytest.mark.parametrize("key", L.RICH, ids=str)
def test_rich(key):
    cs = L.rich(*key)
    r = L.ref(("rich",) + key, cs)
    assert (cs["run"], r["status"], r["kind"]) == (L.UNBOUNDED, L.OPTIMAL, L.RAY)
    assert np.count_nonzero(r["ray"]) == key[0] + 1
    BC.check(cs, r)


@pytest.mark.parametrize("key", L.CONTRA, ids=str)
def test_contra(key):
    cs = L.contra(*key)
    r = L.ref(("contra",) + key, cs)
    assert (cs["run"], r["status"], r["kind"], r["index"]) == (L.INFEASIBLE, L.OPTIMAL, L.FARKAS, -1)
    assert _artificials(cs) == 1
    assert abs(r["value"] + 1.0) < 1e-6
    BC.check(cs, r)


@pytest.mark.parametrize("key", L.UNREACH, ids=str)
def test_unreach(key):
    cs = L.unreach(*key)
    r = L.ref(("unreach",) + key, cs)
    assert (cs["run"], r["status"], r["kind"]) == (L.INFEASIBLE, L.OPTIMAL, L.FARKAS)
    assert _artificials(cs) == 0
    assert cs["dual_pivots"] >= 10
    t = r["index"]
    assert t >= 0
    x, j = _xb(cs)[t], cs["basis"][t]
    if key[4] == "below":
        assert x < cs["lo"][j] - 1e-6
    else:
        assert np.isfinite(cs["hi"][j]) and x > cs["hi"][j] + 1e-6
    BC.check(cs, r)


def test_unreach_has_both_sides():
    assert {k[4] for k in L.UNREACH} == {"below", "above"} and {k[3] for k in L.UNREACH} == {"raise", "lower"}


@pytest.mark.parametrize("key", L.TIE_DUAL, ids=str)
def test_tie_dual(key):
    cs = L.tie_dual(*key)
    ex, nb, alpha = cs["expect"], cs["nonbasic"], cs["alpha"]
    t1, t2, t3, t4 = ex["t"]
    assert np.array_equal(np.linalg.solve(cs["A"][:, cs["basis"]], cs["A"][:, nb]), alpha)   # exact data
    x, L_, H_ = _xb(cs), cs["lo"][cs["basis"]], cs["hi"][cs["basis"]]
    violated = np.flatnonzero((x < L_ - EPS) | (x > H_ + EPS))
    assert violated.tolist() == [t1, t2, t3, t4]
    assert x[t1] == L_[t1] - 1 and x[t2] == L_[t2] - 1 and x[t4] == L_[t4] - 1
    assert x[t3] == (H_[t3] + 1 if ex["side"] == "above" else L_[t3] - 1)
    flagged = cs["at_upper"][nb] == 1
    fails = {}
    for t in (t1, t2, t3, t4):
        g = -alpha[t] if (t == t3 and ex["side"] == "above") else alpha[t]
        fails[t] = nb[np.where(flagged, g > EPS, g < -EPS)]
    assert fails[t1].tolist() == [ex["spoiled"][t1]] and fails[t2].tolist() == [ex["spoiled"][t2]]
    assert fails[t1][0] // 256 != fails[t2][0] // 256
    assert len(fails[t3]) == 0 and len(fails[t4]) == 0
    for eps in (EPS, 0.0):
        r = L.ref(("tie_dual",) + key, cs, eps)
        assert (r["status"], r["kind"], r["index"], r["value"]) == (L.OPTIMAL, L.FARKAS, t3, -1.0)
        BC.check(cs, r)
    # the eps edge: a tolerance equal to the spoiling magnitude lets the spoiled rows pass, and the first one wins
    r = L.ref(("tie_dual",) + key, cs, L.SPOIL)
    assert (r["status"], r["kind"], r["index"], r["value"]) == (L.OPTIMAL, L.FARKAS, t1, -1.0)
    r = L.ref(("tie_dual",) + key, cs, np.nextafter(L.SPOIL, 0.0))
    assert (r["kind"], r["index"]) == (L.FARKAS, t3)


def test_tie_dual_has_both_sides():
    assert {L.tie_dual(*k)["expect"]["side"] for k in L.TIE_DUAL} == {"below", "above"}
    assert {L.tie_dual(*k)["expect"]["side"] for k in L.TIE_DUAL if k[1:] == (257, 1030)} == {"below", "above"}


@pytest.mark.parametrize("key", L.TIE_RAY, ids=str)
def test_tie_ray(key):
    cs = L.tie_ray(*key)
    ex = cs["expect"]
    j1, j2, j3, j4 = ex["j"]
    s = 1.0 if key[3] else -1.0
    assert j1 < j2 < j3 < j4 and j3 // 256 < j4 // 256
    x, L_, H_ = _xb(cs), cs["lo"][cs["basis"]], cs["hi"][cs["basis"]]
    assert ((x >= L_) & (x <= H_)).all()
    for eps in (0.0, EPS):
        r = L.ref(("tie_ray",) + key, cs, eps)
        assert (r["status"], r["kind"], r["index"], r["value"]) == (L.OPTIMAL, L.RAY, j3, 3.0 * s)
        BC.check(cs, r)
    # the eps edge: a tolerance equal to |d_j3| disqualifies j3, and j4 is next
    r = L.ref(("tie_ray",) + key, cs, 3.0)
    assert (r["status"], r["kind"], r["index"], r["value"]) == (L.OPTIMAL, L.RAY, j4, 4.0 * s)
    r = L.ref(("tie_ray",) + key, cs, np.nextafter(3.0, 0.0))
    assert (r["kind"], r["index"]) == (L.RAY, j3)


def test_crossed_bounds_come_before_a_repeated_index():
    cs = L.unreach(160, 320, 1, "raise")
    A, b, c, lo, hi, basis, up = L.at(cs)
    j = int(np.flatnonzero(np.isfinite(hi) & (np.asarray(up) == 0))[0])
    hi2 = np.array(hi)
    hi2[j] = lo[j] - 0.25
    rep = np.array(basis)
    rep[3] = rep[0]
    assert CR.certificate(A, b, c, lo, hi2, basis, up, cs["maximize"])["status"] == L.INFEASIBLE
    assert CR.certificate(A, b, c, lo, hi, rep, up, cs["maximize"])["status"] == L.SINGULAR
    assert CR.certificate(A, b, c, lo, hi2, rep, up, cs["maximize"])["status"] == L.INFEASIBLE
