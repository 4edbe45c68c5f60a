"""Depth-first branch-and-bound without a GPU: tests/ref/mip_ref.c against an enumeration of the integer points,
against resolve_ref.c with an all-zero mask, on mixed-integer problems, and the argument checks of the reference and
of the C ABI (no context needed)."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import mip_ref as M
from tests import resolve_ref as R

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = 0, 1, 2, 3, 4, 5


def _case(s):
    rng = np.random.default_rng(1000 + s)
    m, k = int(rng.integers(2, 7)), int(rng.integers(4, 11))
    return M.knapsack(s, m, k, box=2 if k > 7 else 3), k


@pytest.mark.parametrize("s", range(64))
def test_pure_integer_matches_enumeration(s):
    (A, b, c, basis, mask), k = _case(s)
    r = M.mip(A, b, c, basis, mask, True, k)
    best, _ = M.brute_force(A[:, :k], b, c[:k])
    if best is None:
        assert r["status"] == INFEASIBLE and r["found"] == 0
        return
    assert r["status"] == OPTIMAL and r["found"] == 1
    assert abs(r["obj"] - best) <= 1e-9 * max(1.0, abs(best))
    assert r["bound"] == r["obj"]
    x = r["x"]
    assert np.all(np.abs(x - np.round(x)) <= 1e-6)
    assert np.all(A[:, :k] @ x <= b + 1e-7)


def test_infeasible_integer_program():
    # 2 x0 + 2 x1 = 1 has no integer point; its relaxation is feasible
    A = np.array([[2.0, 2.0, 0.0, 0.0], [1.0, 1.0, 0.0, 1.0]])
    r = M.mip(A, [1.0, 5.0], [1.0, 1.0, 0.0, 0.0], [0, 3], [1, 1, 0, 0], True, 2)
    assert r["status"] == INFEASIBLE and r["found"] == 0
    assert np.isnan(r["obj"]) and np.all(np.isnan(r["x"])) and np.isnan(r["bound"])
    assert r["stats"][0] > 1


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("maximize", [True, False])
def test_zero_mask_is_the_resolve(seed, maximize):
    A, b, c, basis = capi.gen_lp(seed, 8, 20)
    if not maximize:
        c = -c
    b2 = R.scale_rows(seed, b)   # often primal infeasible: the dual branch
    for bb in (b, b2):
        r = M.mip(A, bb, c, basis, np.zeros(20, np.int32), maximize, 12)
        q = R.resolve(A, bb, c, basis, maximize, 12)
        assert r["status"] == q["status"]
        assert r["stats"][0] == 1 and r["stats"][1:3] == q["iters"] and r["stats"][3] == 0
        if q["status"] == OPTIMAL:
            assert r["found"] == 1
            assert np.array_equal(r["x"], q["x"]) and r["obj"] == q["obj"] and r["bound"] == q["obj"]


@pytest.mark.parametrize("s", range(16))
def test_mixed_integer_keeps_slacks_continuous(s):
    (A, b, c, basis, mask), k = _case(s)
    half = mask.copy()
    half[k // 2:] = 0   # the second half of the columns and the slacks continuous
    r = M.mip(A, b, c, basis, half, True, k + A.shape[0])
    pure = M.mip(A, b, c, basis, mask, True, k + A.shape[0])
    root = M.mip(A, b, c, basis, np.zeros_like(mask), True, k + A.shape[0])
    assert r["status"] == OPTIMAL
    x = r["x"]
    assert np.all(np.abs(x[:k // 2] - np.round(x[:k // 2])) <= 1e-6)
    assert np.allclose(A @ x, b, atol=1e-7) and np.all(x >= -1e-9)
    assert root["obj"] + 1e-9 >= r["obj"]
    if pure["status"] == OPTIMAL:
        assert r["obj"] + 1e-9 >= pure["obj"]


def test_limits_keep_the_incumbent():
    (A, b, c, basis, mask), k = _case(3)
    full = M.mip(A, b, c, basis, mask, True, k)
    assert full["status"] == OPTIMAL and full["stats"][0] > 3
    lim = M.mip(A, b, c, basis, mask, True, k, max_nodes=3)
    assert lim["status"] == ITER_LIMIT and lim["stats"][0] == 3
    assert not (lim["bound"] < full["obj"])
    shallow = M.mip(A, b, c, basis, mask, True, k, max_depth=0)
    assert shallow["status"] == ITER_LIMIT and shallow["stats"][0] == 1 and shallow["found"] == 0
    assert shallow["bound"] >= full["obj"]


def test_reference_refuses_bad_arguments():
    (A, b, c, basis, mask), k = _case(0)
    assert M.mip(A, b, c, basis, mask, True, k)["status"] == OPTIMAL
    bad = [dict(max_depth=-1), dict(max_depth=65), dict(int_tol=0.5), dict(int_tol=-1e-3), dict(gap=-1.0),
           dict(max_nodes=0)]
    for kw in bad:
        assert M.mip(A, b, c, basis, mask, True, k, **kw)["status"] == BAD_ARG, kw
    m2 = mask.copy()
    m2[0] = 2
    assert M.mip(A, b, c, basis, m2, True, k)["status"] == BAD_ARG
    m3 = mask.copy()
    m3[k] = 1   # a slack column beyond n_orig
    assert M.mip(A, b, c, basis, m3, True, k)["status"] == BAD_ARG
    b2 = basis.copy()
    b2[0] = A.shape[1]
    assert M.mip(A, b, c, b2, mask, True, k)["status"] == BAD_ARG


def test_capi_refuses_without_a_context():
    lib = capi.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    z = np.zeros(8)
    zi = np.zeros(8, np.int32)
    d, i = z.ctypes.data_as(dp), zi.ctypes.data_as(ip)
    assert lib.lp_mip_solve(None, d, 2, 4, d, d, i, 1, 2, i, 1e-9, 1e-6, 1e-9, 4, 10, 10, d, d, d, i, i) == BAD_ARG
    assert lib.lp_mip_solve_batched(None, 1, d, 2, 4, d, d, i, 1, 2, i, 1e-9, 1e-6, 1e-9, 4, 10, 10, d, d, d, i, i,
                                    i) == BAD_ARG
    assert lib.lp_batched_mip(None, i, 1e-9, 1e-6, 1e-9, 4, 10, 10, d, d, d, i, i, i) == BAD_ARG


def test_fits_predicate():
    lib = capi.load()
    assert lib.lp_mip_fits(16, 40, 24) == 1
    assert lib.lp_mip_fits(64, 192, 0) == 1
    assert lib.lp_mip_fits(16, 40, 65) == 0 and lib.lp_mip_fits(16, 40, -1) == 0
    assert lib.lp_mip_fits(0, 40, 4) == 0 and lib.lp_mip_fits(8, 4, 4) == 0
    assert lib.lp_mip_fits(120, 240, 32) == 0   # the tableau alone is past 160 KB


def test_mask_length_is_checked():
    with pytest.raises(ValueError):
        capi._mask(np.ones(3), 4)
