"""lp_simplex_bounded_large without a GPU: the entry is declared, bound and exported, it refuses bad arguments before
touching a device, and the inputs of tests/test_gpu_bounded_large.py reach what that file claims for them, on the
reference (tests/ref/bounded_ref.c) alone, so that the GPU comparisons cannot pass on vacuous inputs."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import build, capi
from tests import bounded_large_cases as K
from tests import bounded_ref as R


def test_entry_is_declared_bound_and_exported():
    assert "lp_simplex_bounded_large" in capi.SIGNATURES
    assert capi.SIGNATURES["lp_simplex_bounded_large"] == capi.SIGNATURES["lp_simplex_bounded"]
    build.build_hip()
    assert hasattr(C.CDLL(build.HIP_LIB), "lp_simplex_bounded_large")
    assert callable(getattr(capi.Context, "bounded_large"))


def test_refuses_without_a_context():
    lib = capi.load()
    d = np.zeros(16).ctypes.data_as(C.POINTER(C.c_double))
    i = np.zeros(16, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert lib.lp_simplex_bounded_large(None, d, 2, 4, d, d, d, d, 1, 4, 1e-9, 10, d, i, i, d, i) == R.BAD_ARG


@pytest.mark.parametrize("m,n", [(6, 16), (32, 96), (64, 192)])
def test_lds_shapes_flip_and_pivot_in_both_phases(m, n):
    lib = capi.load()
    assert lib.lp_simplex_bounded_fits(m, n) == 1
    for mx in (True, False):
        hit = False
        for seed in (1, 2, 3):
            A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, mx)
            r = K.ref(("lds", m, n, seed, mx), A, b, c, lo, hi, mx, n - m)
            hit |= r["status"] == R.OPTIMAL and r["iters"][0] > 0 and r["iters"][2] > 0 and r["iters"][3] > 0
        assert hit


@pytest.mark.parametrize("m,n,kind,seed", K.BEYOND_CASES)
def test_shapes_beyond_the_lds_fit(m, n, kind, seed):
    # (67 x 201 still fits LDS: it is in this list for its odd tableau width, 67 + 201 + 1 = 269 columns padded to 272)
    assert capi.load().lp_simplex_bounded_fits(m, n) == int((m, n) == (67, 201))
    A, b, c, lo, hi, mx = K.boxed(m, n, kind, seed)
    r = K.ref(("beyond", m, n, kind, seed), A, b, c, lo, hi, mx, n - m)
    want = {"mixed": (R.OPTIMAL, R.UNBOUNDED, R.INFEASIBLE), "box": (R.OPTIMAL,), "unbounded": (R.UNBOUNDED,),
            "infeasible": (R.INFEASIBLE,), "crossed": (R.INFEASIBLE,)}[kind]
    assert r["status"] in want
    if kind == "crossed":
        assert np.any(hi < lo) and r["iters"] == [0, 0, 0, 0] and np.array_equal(r["basis"], n + np.arange(m))
    else:
        assert not np.any(hi < lo)
    if kind in ("mixed", "box", "unbounded"):
        assert r["iters"][0] > 0 and r["iters"][3] > 0
        if r["status"] != R.INFEASIBLE:
            assert r["iters"][2] > 0
    if (m, n, kind, seed) in K.BEYOND:
        status, iters = K.BEYOND[(m, n, kind, seed)]
        assert r["status"] == status
        if iters is not None:
            assert r["iters"] == iters
    if (m, n, kind, seed) == (160, 320, "box", 1):
        assert int(r["at_upper"].sum()) == 101


@pytest.mark.parametrize("kind,seed", sorted(K.TALL))
def test_more_rows_than_selector_threads(kind, seed):
    m, n = K.TALL_SHAPE
    assert m > 1024
    A, b, c, lo, hi, mx = K.boxed(m, n, kind, seed)
    r = K.ref(("tall", kind, seed), A, b, c, lo, hi, mx, n - m, max_iter=K.TALL_MAX_ITER)
    assert r["status"] == R.ITER_LIMIT and r["iters"] == K.TALL[(kind, seed)]
    assert sum(r["iters"]) == K.TALL_MAX_ITER   # the limit fell in phase I: pivots plus flips


@pytest.mark.parametrize("seed", sorted(K.SINGULAR_FLIPS))
def test_duplicated_row_is_singular(seed):
    A, b, c, lo, hi, mx = K.singular(seed)
    r = K.ref(("singular", seed), A, b, c, lo, hi, mx)
    assert r["status"] == R.SINGULAR and r["iters"][3] == K.SINGULAR_FLIPS[seed]
    assert int((r["basis"] >= A.shape[1]).sum()) == 1   # one artificial is left basic


@pytest.mark.parametrize("seed", sorted(K.DRIVEOUT_PIVOTS))
def test_driveout_cases_drive_out(seed):
    A, b, c, lo, hi, mx = K.driveout(seed)
    r = K.ref(("driveout", seed), A, b, c, lo, hi, mx)
    assert r["status"] == R.OPTIMAL and r["iters"][1] == K.DRIVEOUT_PIVOTS[seed]
    assert np.isfinite(hi).any() and r["iters"][3] == 0


@pytest.mark.parametrize("key", sorted(K.DRIVEOUT_FLIP))
def test_driveout_with_flip_cases(key):
    A, b, c, lo, hi, mx = K.driveout_with_flip(*key)
    r = K.ref(("driveout_flip",) + key, A, b, c, lo, hi, mx)
    assert r["status"] == R.OPTIMAL and r["iters"] == K.DRIVEOUT_FLIP[key]
    assert r["iters"][1] > 0 and r["iters"][3] > 0


def test_iteration_limit_sweeps_mix_flips_and_pivots():
    for (m, n, top) in ((6, 16, 12), (67, 201, 6)):
        A, b, c, lo, hi, mx = K.boxed(m, n, "mixed", 1)
        seen = [K.ref(("limit", m, n, k), A, b, c, lo, hi, mx, n - m, max_iter=k) for k in range(1, top + 1)]
        assert any(r["status"] == R.ITER_LIMIT for r in seen)
        assert any(r["iters"][3] > 0 for r in seen) and any(r["iters"][0] > 0 for r in seen)
        if m == 6:   # the sweep crosses from a limit in phase I to phase II
            assert seen[0]["iters"][2] == 0 and any(r["iters"][2] > 0 or r["status"] == R.OPTIMAL for r in seen)
