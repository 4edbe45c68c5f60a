"""lp_basis_bounded_duals_large and lp_basis_bounded_ranging_large without a GPU: the entries are declared, bound and
exported, they refuse a missing context before touching a device, and the inputs of
tests/test_gpu_bounded_sens_large.py reach what that file claims for them, on the references alone
(tests/ref/bounded_ref.c for the solves, tests/ref/bounded_sens_ref.c for the analyses, and for the tie cases an exact
numpy model of the integer data), so that the GPU comparisons cannot pass on vacuous inputs."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import build, capi
from tests import bounded_sens_large_cases as L
from tests import bounded_sens_ref as S

OPTIMAL, BAD_ARG = 0, 5
ENTRIES = {"lp_basis_bounded_duals_large": ("lp_basis_bounded_duals", "bounded_duals_large"),
           "lp_basis_bounded_ranging_large": ("lp_basis_bounded_ranging", "bounded_ranging_large")}


def test_entries_are_declared_bound_and_exported():
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name, (plain, method) in ENTRIES.items():
        assert name in capi.SIGNATURES
        assert capi.SIGNATURES[name] == capi.SIGNATURES[plain]
        assert hasattr(lib, name)
        assert callable(getattr(capi.Context, method))


def test_refusal_without_a_context():
    lib = capi.load()
    d = np.zeros(16).ctypes.data_as(C.POINTER(C.c_double))
    i = np.zeros(16, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert lib.lp_basis_bounded_duals_large(None, d, 2, 4, d, d, d, d, i, i, d, d, d, d) == BAD_ARG
    assert lib.lp_basis_bounded_ranging_large(None, d, 2, 4, d, d, d, d, i, i, 1, 1e-9, d, i, i, d, i) == BAD_ARG


@pytest.mark.parametrize("m,n,kind,seed", L.SOLVED)
def test_solved_cases_are_optimal_with_upper_flags_and_upper_sides(m, n, kind, seed):
    assert capi.load().lp_basis_bounded_fits(m, n) == int((m, n) == (67, 201))
    A, b, c, lo, hi, mx = L.Q.boxed(m, n, kind, seed)
    sol = L.solved_ref(m, n, kind, seed)
    assert sol["status"] == OPTIMAL
    at = (A, b, c, lo, hi, sol["basis"], sol["at_upper"])
    key = (m, n, kind, seed)
    g, q = L.duals(key, *at), L.ranging(key, *at, maximize=mx)
    assert g["status"] == OPTIMAL and q["status"] == OPTIMAL
    assert 3 <= int(np.sum(sol["at_upper"])) <= 101
    assert 2 <= int(np.sum(q["b_side"] == 1)) <= 63


def _winners(values, ok, want_max):
    """Indices of `ok` whose value is the extreme one (exact ties), ascending; empty without a candidate."""
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return idx
    best = values[idx].max() if want_max else values[idx].min()
    return idx[values[idx] == best]


@pytest.mark.parametrize("seed,m,n", L.TIES)
def test_tie_cases_tie(seed, m, n):
    """The exact model: B^-1 = round(inv(B)) has entries 0 and +-1, so xB, y, d and B^-1 A are integers and every ratio
    is the correctly rounded quotient of two small integers, as in the reference."""
    A, b, c, lo, hi, basis, up = L.tie(seed, m, n)
    eps = 1e-9
    Binv = np.rint(np.linalg.inv(A[:, basis]))
    assert np.array_equal(Binv @ A[:, basis], np.eye(m)) and set(np.unique(Binv).tolist()) <= {-1.0, 0.0, 1.0}
    nonbasic = np.ones(n, bool)
    nonbasic[basis] = False
    v = np.where(nonbasic, np.where(up == 1, hi, lo), 0.0)
    xB = Binv @ (b - A @ v)
    Lb, Hb = lo[basis], hi[basis]
    assert np.all((xB - Lb >= 0) & (xB - Lb <= 2))
    q = {mx: L.ranging(("tie", seed), A, b, c, lo, hi, basis, up, maximize=mx, eps=eps) for mx in (False, True)}
    assert q[False]["status"] == OPTIMAL and q[True]["status"] == OPTIMAL
    # ---- RHS ranges: the lower end of row i is a max over positions t (each has at most one candidate there)
    tied = first_not_smallest = 0
    for i in range(m):
        beta = Binv[:, i]
        for end, want_max in ((0, True), (1, False)):
            # the L candidate goes to the lower end under beta > 0, the H candidate (H finite) under beta < 0
            use_L = (beta > eps) if end == 0 else (beta < -eps)
            use_H = ((beta < -eps) if end == 0 else (beta > eps)) & np.isfinite(Hb)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(use_L, (Lb - xB) / beta, (Hb - xB) / beta)
            win = _winners(ratio, use_L | use_H, want_max)
            leave = -1 if len(win) == 0 else int(basis[win[0]])
            assert q[False]["b_leave"][i, end] == leave   # the first position, on both ends of every row
            if end == 0 and len(win) > 1:
                tied += 1
                first_not_smallest += int(basis[win[0]] != basis[win].min())
    assert 2 * tied >= m and 2 * first_not_smallest >= tied
    # ---- cost ranges: some basic column's winning ratio is attained in more than one 256-column chunk
    y = Binv.T @ c[basis]
    d = c - A.T @ y
    alpha = Binv @ A
    for mx in (False, True):
        sense = mx != (up == 1)
        chunks = 0
        for t in range(m):
            a = alpha[t]
            live = nonbasic & (np.abs(a) > eps)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = d / a
            lower = live & ((a > eps) == sense)
            for end, ok, want_max in ((0, lower, True), (1, live & ~lower, False)):
                win = _winners(ratio, ok, want_max)
                enter = -1 if len(win) == 0 else int(win[0])
                assert q[mx]["c_enter"][basis[t], end] == enter
                chunks += len(win) > 1 and len(set((win // 256).tolist())) > 1
        assert chunks >= 1


def test_the_reference_is_exact_on_a_tie_case():
    """On integer data the reference's x, y, d and w are the model's exactly."""
    A, b, c, lo, hi, basis, up = L.tie(1, 150, 600)
    g = L.duals(("tie", 1), A, b, c, lo, hi, basis, up)
    assert g["status"] == OPTIMAL
    Binv = np.rint(np.linalg.inv(A[:, basis]))
    nonbasic = np.ones(600, bool)
    nonbasic[basis] = False
    v = np.where(nonbasic, np.where(up == 1, hi, lo), 0.0)
    x = v.copy()
    x[basis] = Binv @ (b - A @ v)
    y = Binv.T @ c[basis]
    d = np.where(nonbasic, c - A.T @ y, 0.0)
    assert np.array_equal(g["x"], x) and np.array_equal(g["y"], y) and np.array_equal(g["d"], d)
    assert g["w"] == b @ y + d @ v == c @ x
