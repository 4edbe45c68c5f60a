"""The tolerance families of tests/tolcases.py on the oracle alone (no GPU): they must be what the GPU tests
(tests/test_gpu_tolerance.py) need them to be, or those tests would pass without looking at anything.

  - every near-tie and tiny-entry case is eps-sensitive: its oracle trace at eps = 0 differs from the one at 1e-9, and
    every case that also runs at LARGE_EPS has a trace there that differs from the one at 1e-9;
  - the first-pivot near-tie family is adversarial for a ranking by approximate quotients;
  - the power-of-two scalings are exact symmetries of the oracle at eps = 0."""
import numpy as np
import pytest

from oracle import pyoracle as o
from tests import tolcases as T

_SENSITIVE = ("near_rows", "near_cols", "tiny")


def _trace(A, b, c, basis, eps, max_iter):
    m, n = A.shape
    return o.simplex_tableau(A, b, c, basis, True, n - m, eps=eps, max_iter=max_iter, trace_cap=1 << 14)


@pytest.mark.parametrize("case", T.single_cases(), ids=T.case_id)
def test_cases_are_eps_sensitive(case):
    fam, seed, m, n, idx, max_iter, large = case
    A, b, c, basis = T.family_case(fam, seed, m, n, idx)
    r9 = _trace(A, b, c, basis, 1e-9, max_iter)
    if fam in _SENSITIVE:
        r0 = _trace(A, b, c, basis, 0.0, max_iter)
        assert r0["trace"] != r9["trace"]
    if large:
        r2 = _trace(A, b, c, basis, T.LARGE_EPS, max_iter)
        assert r2["trace"] != r9["trace"]


@pytest.mark.parametrize("u", T.TINY)
def test_tiny_entry_pivots_first_at_eps_zero(u):
    """The degenerate row with the tiny entry leaves at the first pivot exactly when eps < u."""
    m, n = 64, 160
    A, b, c, basis = T.tiny_entry(5, m, n, u, 63)
    q = int(np.flatnonzero(b == 0.0)[0])
    e = int(np.argmax(c))
    assert A[q, e] == u
    for eps, takes in ((0.0, True), (np.nextafter(u, 0.0) if u > 5e-324 else 0.0, True), (u, False), (1e-9, False)):
        r = _trace(A, b, c, basis, eps, 1)
        assert r["trace"][0][0] == e
        assert (r["trace"][0][1] == q) == takes, (eps, r["trace"])


def _emulated_fast_pick(x, u, eps):
    """The chip-resident fast path on one column, with RN(1/u) for the device's refined reciprocal: q~ = x * RN(1/u);
    the first index of the approximate minimum if the slack verdict on the rows in front of it holds and
    |q~| < 2^15, else the exact chain (what the kernel's replay does).  The device's reciprocal may differ from
    RN(1/u) by an ulp: the family is large, not hand-picked, so that the rate does not hinge on that ulp."""
    S = 2.0 ** -48
    mask = u > eps
    exact = o.chain_select(x / np.where(mask, u, 1.0), mask, want_max=False, eps=eps)[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        qa = np.where(mask, x * (1.0 / u), np.inf)
    qa = np.where(np.isnan(qa), np.inf, qa)
    L = int(np.argmin(qa))
    M = qa[L]
    if not np.isfinite(M):
        return exact, exact
    front = qa[:L]
    ok = np.all((M + eps) + S * abs(M) < front - S * np.abs(front)) and abs(M) < 32768.0
    return (L if ok else exact), exact


def test_first_pivot_family_defeats_approximate_ranking():
    """At eps = 0 at least 5 % of the family's first ratio tests pick another row under the emulated fast path than
    under the exact chain (orc_chain_select).  At eps = 1e-9 none does: the emulation is the kernel's argument."""
    A, b, c, basis = T.first_pivot_pairs(0, 400)
    count, m, n = A.shape
    wrong0 = wrong9 = 0
    for k in range(count):
        e = int(np.argmax(c[k]))
        fast, exact = _emulated_fast_pick(b[k], A[k][:, e], 0.0)
        wrong0 += fast != exact
        fast, exact = _emulated_fast_pick(b[k], A[k][:, e], 1e-9)
        wrong9 += fast != exact
    assert wrong0 >= 0.05 * count, (wrong0, count)
    assert wrong9 == 0


def test_first_pivot_family_first_ratio_test_is_a_near_tie():
    """Each LP's first pivot at eps = 0 takes the twin BEHIND the first minimum; at 1e-9 the front row."""
    A, b, c, basis = T.first_pivot_pairs(1, 48)
    count, m, n = A.shape
    for k in range(count):
        r0 = _trace(A[k], b[k], c[k], basis[k], 0.0, 1)
        r9 = _trace(A[k], b[k], c[k], basis[k], 1e-9, 1)
        (e0, l0), (e9, l9) = r0["trace"][0], r9["trace"][0]
        assert e0 == e9 and l0 > l9
        u = A[k][:, e0]
        assert 0.0 < (b[k][l9] / u[l9] - b[k][l0] / u[l0]) <= 4 * np.spacing(b[k][l9] / u[l9])


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("kb,kc", T.POW2)
@pytest.mark.parametrize("fam,idx,m,n", [("near_rows", 0, 64, 160), ("near_cols", 5, 200, 600), ("ties", 0, 64, 160)])
def test_pow2_invariance_in_the_oracle(fam, idx, m, n, kb, kc):
    """At eps = 0: same trace and basis, x exactly 2^kb x, obj exactly 2^(kb + kc) obj."""
    A, b, c, basis = T.family_case(fam, 3, m, n, idx)
    r = o.simplex_tableau(A, b, c, basis, True, n - m, eps=0.0, trace_cap=1 << 14)
    A2, b2, c2 = T.pow2_scaled(A, b, c, kb, kc)
    s = o.simplex_tableau(A2, b2, c2, basis, True, n - m, eps=0.0, trace_cap=1 << 14)
    assert r["status"] == s["status"] == o.OPTIMAL and r["iters"] > 0
    assert s["trace"] == r["trace"]
    assert np.array_equal(s["basis"], r["basis"])
    assert np.array_equal(_bits(s["x"]), _bits(r["x"] * 2.0 ** kb))
    assert _bits(s["obj"]) == _bits(r["obj"] * 2.0 ** (kb + kc))


def test_cases_are_deterministic():
    for fam in T.FAMILIES:
        a = T.family_case(fam, 7, 64, 160, 3)
        b = T.family_case(fam, 7, 64, 160, 3)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
