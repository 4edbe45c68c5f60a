"""CPU-only checks of RHS and cost ranging at a basis: the test restatement (tests/ref/ranging_ref.c) against plain
numpy formulas, its pieces bit for bit against the duals restatement and the oracle's crash, the in-place crash
against the explicit [B | I | b] form, HiGHS objectives on both sides of every finite end (the golden cases), ties,
infinite and zero-width ends, the statuses, and the C ABI's argument checks without a device."""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import duals_ref as D
from tests import lpcases
from tests import ranging_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-9


def _lp(seed):
    """(A, b, c, starting basis, maximize), as tests/test_duals_cpu.py."""
    m = 2 + seed % 17
    if seed % 2:
        A, b, c, basis = lpcases.general_lp(seed, m, 2 * m + seed % 5)
        return A, b, c, basis, bool(seed % 4 == 1)
    A, b, c, basis = capi.gen_lp(seed, m, 2 * m + 3 + seed % 7)
    return A, b, c, basis, True


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _numpy_ranges(A, b, c, basis, maximize, eps=EPS):
    """The same ranges from np.linalg.inv (close to the reference, not bit-exact)."""
    m, n = A.shape
    Binv = np.linalg.inv(A[:, basis])
    xB = Binv @ b
    y = np.linalg.solve(A[:, basis].T, c[basis])
    d = c - A.T @ y
    d[basis] = 0.0
    nonbasic = np.setdiff1d(np.arange(n), basis)
    alpha = Binv @ A
    b_lo, b_hi = np.empty(m), np.empty(m)
    for i in range(m):
        beta = Binv[:, i]
        r = -xB / np.where(beta == 0, 1, beta)
        b_lo[i] = b[i] + r[beta > eps].max() if (beta > eps).any() else -np.inf
        b_hi[i] = b[i] + r[beta < -eps].min() if (beta < -eps).any() else np.inf
    c_lo, c_hi = np.empty(n), np.empty(n)
    for j in nonbasic:
        c_lo[j], c_hi[j] = (-np.inf, c[j] - d[j]) if maximize else (c[j] - d[j], np.inf)
    for t, q in enumerate(basis):
        a = alpha[t, nonbasic]
        rho = d[nonbasic] / np.where(a == 0, 1, a)
        pos = rho[a > eps].max() if (a > eps).any() else None
        neg = rho[a < -eps].min() if (a < -eps).any() else None
        if not maximize:   # the sides swap
            pos = rho[a > eps].min() if (a > eps).any() else None
            neg = rho[a < -eps].max() if (a < -eps).any() else None
            pos, neg = neg, pos
        c_lo[q] = c[q] + pos if pos is not None else -np.inf
        c_hi[q] = c[q] + neg if neg is not None else np.inf
    return b_lo, b_hi, c_lo, c_hi


def _close(a, b, scale):
    inf = np.isinf(b)
    assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf])
    assert np.allclose(a[~inf], b[~inf], rtol=1e-9, atol=1e-9 * scale)


@pytest.mark.parametrize("seed", range(30))
def test_matches_numpy_at_the_oracle_optimum(seed):
    A, b, c, basis, mx = _lp(seed)
    q = o.simplex_tableau(A, b, c, basis, mx, A.shape[1])
    B = q["basis"] if q["status"] == o.OPTIMAL else basis
    r = RR.ranging(A, b, c, B, mx)
    assert r["status"] == o.OPTIMAL
    b_lo, b_hi, c_lo, c_hi = _numpy_ranges(A, b, c, B, mx)
    scale = 1 + np.abs(b).max() + np.abs(c).max()
    _close(r["b_lo"], b_lo, scale)
    _close(r["b_hi"], b_hi, scale)
    _close(r["c_lo"], c_lo, scale)
    _close(r["c_hi"], c_hi, scale)
    if q["status"] == o.OPTIMAL:   # the current value lies in its own range
        assert (r["b_lo"] <= b + 1e-9).all() and (b <= r["b_hi"] + 1e-9).all()
        assert (r["c_lo"] <= c + 1e-9).all() and (c <= r["c_hi"] + 1e-9).all()
    # indices: the leaving column is basic, the entering one non-basic, -1 exactly at infinite ends
    for lo, hi, idx in ((r["b_lo"], r["b_hi"], r["b_leave"]), (r["c_lo"], r["c_hi"], r["c_enter"])):
        assert np.array_equal(idx[:, 0] < 0, np.isinf(lo)) and np.array_equal(idx[:, 1] < 0, np.isinf(hi))
    assert set(r["b_leave"][r["b_leave"] >= 0].tolist()) <= set(B.tolist())
    assert not set(r["c_enter"][r["c_enter"] >= 0].tolist()) & set(B.tolist())


@pytest.mark.parametrize("seed", range(20))
def test_reduced_costs_are_the_duals_bits(seed):
    """Non-basic cost ends are c - d with d of duals_ref.c, bit for bit."""
    A, b, c, basis, mx = _lp(seed)
    r = RR.ranging(A, b, c, basis, mx)
    g = D.duals(A, b, c, basis)
    nb = np.setdiff1d(np.arange(A.shape[1]), basis)
    end = r["c_hi"] if mx else r["c_lo"]
    assert np.array_equal(_bits(end[nb]), _bits(c[nb] - g["d"][nb]))
    assert np.array_equal(r["c_enter"][nb, 1 if mx else 0], nb)


@pytest.mark.parametrize("seed", range(20))
def test_xb_is_the_oracle_crash(seed):
    """xB of the crash on [B | I | b] is the b column of the oracle's crash on [A | b] (same basis) bit for bit."""
    A, b, c, _, mx = _lp(seed)
    m, n = A.shape
    rng = np.random.default_rng(seed)
    basis = rng.choice(n, size=m, replace=False).astype(np.int32)   # not the slack identity: the crash runs
    q = o.simplex_tableau(A, b, c, basis, mx, n, max_iter=0, want_tableau=True)
    st, _, xb = RR.crash(A, b, basis, inplace=False)
    if q["status"] == o.SINGULAR:
        assert st == o.SINGULAR
        return
    assert st == o.OPTIMAL
    assert np.array_equal(_bits(xb), _bits(q["tableau"][:m, n]))


def _sparse_lp(seed, m, n):
    """Integer-valued sparse A with signed entries: many exact zeros, so signed zeros appear in the crash."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, size=(m, n)).astype(np.float64) * (rng.random((m, n)) < 0.4)
    A[:, :m] += np.diag(rng.choice([-2.0, 2.0], size=m))
    b = rng.integers(-5, 6, size=m).astype(np.float64)
    return A, b


@pytest.mark.parametrize("seed", range(40))
def test_in_place_crash_is_the_explicit_form(seed):
    m = 1 + seed % 23
    if seed % 3 == 0:
        A, b = _sparse_lp(seed, m, 2 * m + 3)
    else:
        A, b, _, _ = capi.gen_lp(seed, m, 2 * m + 3)
    rng = np.random.default_rng(100 + seed)
    basis = rng.choice(A.shape[1], size=m, replace=False).astype(np.int32)
    s0, Binv0, x0 = RR.crash(A, b, basis, inplace=False)
    s1, Binv1, x1 = RR.crash(A, b, basis, inplace=True)
    assert s0 == s1
    if s0 == o.OPTIMAL:
        assert np.array_equal(_bits(Binv0), _bits(Binv1))   # signed zeros included
        assert np.array_equal(_bits(x0), _bits(x1))


def test_in_place_crash_keeps_negative_zeros():
    """A case where B^-1 holds -0.0: the in-place form's zero-sign flags are exercised."""
    found = 0
    for seed in range(60):
        A, b = _sparse_lp(seed, 6, 15)
        basis = np.random.default_rng(seed).choice(15, size=6, replace=False).astype(np.int32)
        s0, Binv0, _ = RR.crash(A, b, basis, inplace=False)
        if s0 != o.OPTIMAL:
            continue
        neg = (Binv0 == 0) & np.signbit(Binv0)
        if neg.any():
            found += 1
            assert np.array_equal(_bits(Binv0), _bits(RR.crash(A, b, basis, inplace=True)[1]))
    assert found >= 3


def test_golden_highs_objectives():
    cases = json.load(open(os.path.join(HERE, "golden", "ranging_cases.json")))
    assert len(cases) >= 12 and {g["maximize"] for g in cases} == {True, False}
    for g in cases:
        if g["kind"] == "gen_lp":
            A, b, c, _ = capi.gen_lp(*g["args"])
        else:
            A, b, c, _ = lpcases.min_lp(*g["args"])
        basis = np.array(g["basis"], np.int32)
        mx = g["maximize"]
        r = RR.ranging(A, b, c, basis, mx)
        assert r["status"] == o.OPTIMAL
        x = np.zeros(A.shape[1])
        x[basis] = np.linalg.solve(A[:, basis], b)
        y = D.duals(A, b, c, basis)["y"]
        z = g["obj"]
        assert len(g["points"]) >= 4
        for p in g["points"]:
            k, side = p["k"], p["side"]
            v0 = b[k] if p["what"] == "b" else c[k]
            end = (r["b_lo"], r["b_hi"])[side][k] if p["what"] == "b" else (r["c_lo"], r["c_hi"])[side][k]
            slope = y[k] if p["what"] == "b" else x[k]
            vin, zin = p["inside"]
            vout, zout = p["outside"]
            assert min(v0, end) <= vin <= max(v0, end)                      # inside the reference's range
            assert (vout > end) if side else (vout < end)                   # beyond it
            tol = 1e-7 * (1 + abs(z))
            assert zin is not None and abs(zin - (z + slope * (vin - v0))) <= tol, (g["args"], p)
            if zout is not None:
                assert abs(zout - (z + slope * (vout - v0))) > 10 * tol, (g["args"], p)


def test_ties_take_the_first_index():
    """Two basic rows with equal ratios in the RHS range and two non-basic columns with equal ratios in a cost
    range: the first position / column wins, and a tie between -0.0 and +0.0 keeps the first one's sign."""
    # max x0 + x1 s.t. x0 + s0 = 1, x1 + s1 = 1, x0 + x1 + s2 = 3 at basis (x0, x1, s2)
    A = np.array([[1.0, 0, 1, 0, 0], [0, 1.0, 0, 1, 0], [1.0, 1, 0, 0, 1]])
    b = np.array([1.0, 1.0, 3.0])
    c = np.array([1.0, 1.0, 0, 0, 0])
    basis = np.array([0, 1, 4], np.int32)
    r = RR.ranging(A, b, c, basis, True)
    assert r["status"] == o.OPTIMAL
    assert r["b_lo"][0] == 0.0 and r["b_leave"][0, 0] == 0   # x0 leaves at b0 = 0
    assert r["b_hi"][0] == 2.0 and r["b_leave"][0, 1] == 4   # s2 leaves at b0 = 2
    # degenerate: s2 = 0 when b2 = 2; both x0 and x1 rows give the same ratio for the third row's upper end
    b2 = np.array([1.0, 1.0, 2.0])
    r = RR.ranging(A, b2, c, basis, True)
    assert r["b_hi"][0] == 1.0 and r["b_leave"][0, 1] == 4   # zero-width upper end at the degenerate basis
    assert r["b_lo"][2] == 2.0 and r["b_leave"][2, 0] == 4
    # costs: c = (1, 1); basic x0: d_s0 = -1 with alpha = 1, d_s2 = 0 (s2 basic) -> lower end 1 + max(-1 / 1)
    assert r["c_lo"][0] == 0.0 and r["c_enter"][0, 0] == 2
    assert r["c_hi"][0] == np.inf and r["c_enter"][0, 1] == -1
    # equal ratios on two non-basic columns: column 2 and a copy of it at column 5
    A6 = np.hstack([A, A[:, 2:3]])
    c6 = np.concatenate([c, [0.0]])
    r = RR.ranging(A6, b, c6, basis, True)
    assert r["c_lo"][0] == 0.0 and r["c_enter"][0, 0] == 2   # the first of the two tied columns
    # a tie of -0.0 against +0.0: x_B = 0 for both candidate rows, betas of opposite sign per row
    A0 = np.array([[1.0, 0, 1, 0], [0, -1.0, 0, 1]])
    b0 = np.array([0.0, 0.0])
    r = RR.ranging(A0, b0, np.array([1.0, 1.0, 0, 0]), np.array([0, 1], np.int32), True)
    assert r["b_lo"][0] == 0.0 and not np.signbit(r["b_lo"][0])   # b + (-0.0 / 1 ... ) = 0.0 + -0.0 = +0.0
    assert r["b_leave"][0, 0] == 0


def test_infinite_ends():
    """At the slack basis of a max problem every cost end is infinite on the unbounded side."""
    A, b, c, basis = capi.gen_lp(4, 5, 12)
    r = RR.ranging(A, b, c, basis, True)
    assert r["status"] == o.OPTIMAL
    nb = np.setdiff1d(np.arange(12), basis)
    assert np.isneginf(r["c_lo"][nb]).all() and (r["c_enter"][nb, 0] == -1).all()
    # the slack basis is B = I: the rows' own slack is the only candidate below and nothing bounds above
    assert np.isposinf(r["b_hi"]).all() and (r["b_leave"][:, 1] == -1).all()
    assert np.array_equal(r["b_lo"], np.zeros(5)) and np.array_equal(r["b_leave"][:, 0], basis)
    rmin = RR.ranging(A, b, -c, basis, False)
    assert np.isposinf(rmin["c_hi"][nb]).all() and np.array_equal(rmin["c_enter"][nb, 0], nb)


def test_statuses():
    A, b, c, basis = capi.gen_lp(3, 6, 14)
    Bs = basis.copy()
    Bs[2] = Bs[0]   # repeated column
    r = RR.ranging(A, b, c, Bs)
    assert r["status"] == o.SINGULAR
    assert np.isnan(r["b_lo"]).all() and np.isnan(r["c_hi"]).all() and (r["b_leave"] == -1).all()
    assert (r["c_enter"] == -1).all()
    Bo = basis.copy()
    Bo[1] = A.shape[1]
    assert RR.ranging(A, b, c, Bo)["status"] == o.BAD_ARG
    Bo[1] = -1
    assert RR.ranging(A, b, c, Bo)["status"] == o.BAD_ARG
    for eps in (-1e-12, float("nan")):
        r = RR.ranging(A, b, c, basis, True, eps)
        assert r["status"] == o.BAD_ARG and np.isnan(r["b_lo"]).all()
    assert RR.ranging(A, b, c, basis, True, 0.0)["status"] == o.OPTIMAL


def test_abi_rejects_bad_arguments_without_a_device():
    lib = capi.load()
    m, n, batch = 2, 4, 2
    A = np.zeros(batch * m * n)
    b, c = np.ones(batch * m), np.ones(batch * n)
    basis = np.zeros(batch * m, np.int32)
    rhs, cost = np.zeros(batch * 2 * m), np.zeros(batch * 2 * n)
    rv, cv = np.zeros(batch * 2 * m, np.int32), np.zeros(batch * 2 * n, np.int32)
    st = np.zeros(batch, np.int32)
    dp, ip = capi._d, capi._i
    assert lib.lp_basis_ranging(None, dp(A), m, n, dp(b), dp(c), ip(basis), 1, EPS, dp(rhs), ip(rv), dp(cost),
                                ip(cv)) == capi.BAD_ARG
    assert lib.lp_basis_ranging_batched(None, batch, dp(A), m, n, dp(b), dp(c), ip(basis), 1, EPS, dp(rhs), ip(rv),
                                        dp(cost), ip(cv), ip(st)) == capi.BAD_ARG
    assert lib.lp_batched_ranging(None, EPS, dp(rhs), ip(rv), dp(cost), ip(cv), ip(st)) == capi.BAD_ARG


def test_fits_predicate():
    lib = capi.load()
    assert lib.lp_basis_ranging_fits(64, 192) == 1 and lib.lp_basis_ranging_fits(128, 256) == 1
    assert lib.lp_basis_ranging_fits(512, 1024) == 0 and lib.lp_basis_ranging_fits(0, 4) == 0
    assert lib.lp_basis_ranging_fits(8, 4) == 0
    assert lib.lp_basis_ranging_fits(132, 132) == 1 and lib.lp_basis_ranging_fits(133, 133) == 0


def _two_phase_fits(m, n):
    """lp_batched_two_phase_fits restated (batched_two_phase.hip): the two-phase / re-solve kernels' LDS."""
    W = n + 1
    pitch = W if W & 1 else W + 1
    dbl = 2 + (m + 1) * pitch + W + (m + 1)
    return n >= m and ((dbl * 8 + 4 * (n + m) + 15) & ~15) <= 160 * 1024


def test_fits_covers_the_batched_two_phase_shapes_up_to_m_132():
    lib = capi.load()
    for m in range(1, 133):
        n = m
        while _two_phase_fits(m, n + 1):
            n += 1
        assert _two_phase_fits(m, n)
        for nn in (m, (m + n) // 2, n):
            assert lib.lp_basis_ranging_fits(m, nn) == 1, (m, nn)
    assert _two_phase_fits(140, 140) and not lib.lp_basis_ranging_fits(140, 140)
