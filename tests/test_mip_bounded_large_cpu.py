"""lp_mip_bounded_solve_large without a GPU: the entry is declared, bound and exported, it refuses a missing context
before touching a device, and the inputs of tests/test_gpu_mip_bounded_large.py reach what that file claims for them, on
the references alone (tests/ref/mip_bounded_ref.c for the searches, tests/ref/bounded_resolve_ref.c for the host-driven
search that tells dives from rebuilds), so that the GPU comparisons cannot pass on vacuous inputs.  The recorded results
of the 1100 x 2300 problem are regenerated and compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import build, capi
from tests import bounded_resolve_large_cases as W
from tests import bounded_resolve_ref as BR
from tests import mip_bounded_large_cases as Q
from tests import mip_bounded_ref as R
from tests.test_gpu_mip_bounded import _outcome_cases, _same

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def test_entry_is_declared_bound_and_exported():
    assert "lp_mip_bounded_solve_large" in capi.SIGNATURES
    assert capi.SIGNATURES["lp_mip_bounded_solve_large"] == capi.SIGNATURES["lp_mip_bounded_solve"]
    build.build_hip()
    assert hasattr(C.CDLL(build.HIP_LIB), "lp_mip_bounded_solve_large")
    assert callable(getattr(capi.Context, "mip_bounded_solve_large"))
    assert capi.load().lp_abi_version() == 4


def test_refuses_without_a_context():
    lib = capi.load()
    d = np.zeros(16).ctypes.data_as(C.POINTER(C.c_double))
    i = np.zeros(16, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert lib.lp_mip_bounded_solve_large(None, d, 2, 4, d, d, d, d, i, i, 1, 4, i, 1e-9, 1e-6, 1e-9, 4, 10, 10, d, d, d,
                                          i, i) == BAD_ARG


def test_the_header_points_at_the_entry():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "simplexmethod_amd.h")).read()
    assert "Out of scope on this path" not in text and "lp_mip_bounded_solve_large" in text


@pytest.mark.parametrize("m,n,depth,kind", Q.LDS_SHAPES)
def test_lds_shapes_search(m, n, depth, kind):
    assert capi.load().lp_mip_bounded_fits(m, n, depth) == 1
    searched = infeasible = 0
    for mx in (True, False):
        for seed in range(3):
            for every in (1, 2):
                got = Q.searched(m, n, seed, mx, kind, every, max_depth=depth, max_nodes=Q.LDS_NODES)
                if got is None:
                    continue
                args, r = got
                searched += r["stats"][0] > 1
                if (m, n) == (8, 20):
                    h = Q.host_search(BR.resolve, *args, max_depth=depth, max_nodes=Q.LDS_NODES)
                    assert (h["nodes"], h["dual"], h["deepest"]) == (r["stats"][0], r["stats"][1], r["stats"][4])
                    infeasible += h["infeasible_dives"]
    assert searched >= 2
    if (m, n) == (8, 20):
        assert infeasible >= 1


def test_beyond_the_lds_fit_reaches_what_is_claimed():
    seen = dict(found=0, closed=0, node_limit=0, rebuilds=0)
    for m, n, seed, mx, nodes in Q.BEYOND:
        if (m, n) != (67, 201):   # (that one is here for its odd row length)
            assert capi.load().lp_mip_bounded_fits(m, n, 0) == 0
        kw = dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes)
        args, r = Q.searched(m, n, seed, mx, "mixed", 2, **kw)
        seen["found"] += r["found"]
        seen["closed"] += r["status"] == OPTIMAL and r["stats"][0] > 1
        seen["node_limit"] += r["status"] == ITER_LIMIT and r["stats"][0] == nodes
        if (m, n) != (160, 320):
            continue
        assert (r["status"], r["stats"][0]) == Q.BEYOND_160[(seed, mx)]
        if r["status"] == ITER_LIMIT:
            assert r["found"] and 14 <= r["stats"][4] <= 23 and 285 <= r["stats"][1] <= 362
        # the same nodes by one re-solve per node: which were dives, which rebuilds
        h = Q.host_search(BR.resolve, *args, **kw)
        assert (h["nodes"], h["dual"], h["deepest"]) == (r["stats"][0], r["stats"][1], r["stats"][4])
        assert h["dives"] + h["rebuilds"] + 1 == h["nodes"]
        seen["rebuilds"] += h["rebuilds"]
    assert seen["found"] == len(Q.BEYOND) and seen["closed"] >= 2 and seen["node_limit"] >= 4 and seen["rebuilds"] >= 9


def test_first_children_that_end_infeasible():
    m, n, seed, mx, every, nodes = Q.BEYOND_INFEASIBLE_DIVES
    kw = dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes)
    args, r = Q.searched(m, n, seed, mx, "mixed", every, **kw)
    h = Q.host_search(BR.resolve, *args, **kw)
    assert (h["nodes"], h["dual"], h["deepest"]) == (r["stats"][0], r["stats"][1], r["stats"][4])
    assert h["infeasible_dives"] >= 1 and h["rebuilds"] >= 1 and h["dives"] > h["rebuilds"]


@pytest.mark.parametrize("seed", Q.BOX_SEEDS)
def test_rebuild_heavy_and_dive_only(seed):
    args, r = Q.searched(160, 320, seed, True, "box", 1, max_depth=8, max_nodes=60)
    assert r["status"] == ITER_LIMIT and r["stats"][0] == 60 and r["stats"][4] == 8 and 224 <= r["stats"][1] <= 226
    assert not r["found"] and np.isfinite(r["bound"])
    h = Q.host_search(BR.resolve, *args, max_depth=8, max_nodes=60)
    assert h["nodes"] == 60 and h["rebuilds"] >= 20
    args, r = Q.searched(160, 320, seed, True, "box", 1, max_depth=64, max_nodes=60)
    assert r["stats"][0] == 60 and r["stats"][4] == 59   # 59 levels, 59 first children


def test_tall_fixture_is_the_reference():
    """About 25 s: the root alone takes 4368 primal pivots on a 1101 x 2301 tableau."""
    m, n = Q.TALL_SHAPE
    A, b, c, lo, hi, mask = Q.tall(1)
    assert A.shape == (m, n) and m > 1024 and int(mask.sum()) == Q.TALL_K > 1024
    assert np.array_equal(A[:, n - m:], np.eye(m)) and not np.any(c[n - m:])   # the slack identity, zero costs
    fixture = Q.tall_fixture()
    assert sorted(fixture) == sorted(Q.TALL_RUNS)
    for (depth, nodes), want in fixture.items():
        r = R.mip(*Q.tall_args(1), max_depth=depth, max_nodes=nodes, max_iter=Q.TALL_MAX_ITER)
        _same(r, want)
        assert (r["status"], r["stats"]) == Q.TALL_RUNS[(depth, nodes)]
    # (64, 8): every node after the root is a first child; (2, 6): two of the four are rebuilds, with a crash at m rows
    assert Q.TALL_RUNS[(64, 8)][1][4] == 7 and Q.TALL_RUNS[(2, 6)][1][0] - 1 - Q.TALL_RUNS[(2, 6)][1][4] == 2


@pytest.mark.parametrize("kind", ["bound", "cost"])
def test_zero_mask_starts(kind):
    A, b, c, lo, hi, basis, up, mask = Q.zero_mask_start(kind)
    n = len(c)
    r = BR.resolve(A, b, c, lo, hi, basis, up, True, 160)
    z = R.mip(A, b, c, lo, hi, basis, up, np.zeros(n, np.int32), True, 160)
    assert r["status"] == z["status"] == OPTIMAL and z["stats"] == (1,) + tuple(r["iters"]) + (0,)
    assert np.array_equal(r["x"], z["x"]) and r["obj"] == z["obj"] == z["bound"]
    if kind == "bound":
        assert r["iters"][0] > 0 and r["iters"][1] == 0
        assert R.mip(A, b, c, lo, hi, basis, up, mask, True, 160, max_depth=64, max_nodes=20)["stats"][0] == 20
    else:
        assert r["iters"][0] == 0 and r["iters"][1] > 0 and r["iters"][2] > 0
        rounded = Q.zero_mask_start(kind, rounded=True)
        assert BR.resolve(*rounded[:7], True, 160)["status"] == BAD_ARG


def test_outcomes():
    A, b, c, lo, hi, basis, up, mask, kinds, kw, expect = _outcome_cases()
    assert len(kinds) == 9
    for k, kind in enumerate(kinds):
        assert R.mip(A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, 4, **kw)["status"] == expect[kind]
    cases = {name: start for name, start, _, _ in W.outcomes_160(W.cold_ref(160, 320, 1, True))}
    r = Q.ref(("singular-160",), *cases["singular"], np.zeros(320, np.int32), True, 160)
    assert r["status"] == SINGULAR and r["stats"] == (1, 0, 0, 0, 0) and np.isnan(r["bound"])


def test_deep_case_goes_past_level_64():
    A, b, c, lo, hi, mask, maximize, root = R.deep_case()
    args = (A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, R.DEEP_K)
    r = Q.ref(("deep",), *args, max_depth=1024)
    assert r["status"] == OPTIMAL and r["stats"][4] > 64 and r["stats"][0] > 2000
    h = Q.host_search(BR.resolve, *args, max_depth=1024)
    assert h["nodes"] == r["stats"][0] and h["rebuilds"] > 1000 and h["infeasible_dives"] >= 1


@pytest.mark.parametrize("eps", [0.0, 1e-12])
def test_eps_zero_and_tiny_still_search(eps):
    args, r = Q.searched(67, 201, 1, True, "mixed", 2, eps=eps, max_depth=64, max_nodes=30)
    assert r["stats"][0] == 30 and r["stats"][1] > 0
