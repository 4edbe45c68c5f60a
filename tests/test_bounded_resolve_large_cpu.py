"""lp_simplex_bounded_resolve_large without a GPU: the entry is declared, bound and exported, it refuses a missing
context before touching a device, and the inputs of tests/test_gpu_bounded_resolve_large.py reach what that file claims
for them, on the references (tests/ref/bounded_ref.c for the cold solves, tests/ref/bounded_resolve_ref.c for the
re-solves) alone, so that the GPU comparisons cannot pass on vacuous inputs."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import build, capi
from tests import bounded_resolve_large_cases as Q
from tests import bounded_resolve_ref as W
from tests import resolve_ref

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def test_entry_is_declared_bound_and_exported():
    assert "lp_simplex_bounded_resolve_large" in capi.SIGNATURES
    assert capi.SIGNATURES["lp_simplex_bounded_resolve_large"] == capi.SIGNATURES["lp_simplex_bounded_resolve"]
    build.build_hip()
    assert hasattr(C.CDLL(build.HIP_LIB), "lp_simplex_bounded_resolve_large")
    assert callable(getattr(capi.Context, "bounded_resolve_large"))


def test_refuses_without_a_context():
    lib = capi.load()
    d = np.zeros(16).ctypes.data_as(C.POINTER(C.c_double))
    i = np.zeros(16, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert lib.lp_simplex_bounded_resolve_large(None, d, 2, 4, d, d, d, d, i, i, 1, 4, 1e-9, 10, d, i, i, d,
                                                i) == BAD_ARG


@pytest.mark.parametrize("m,n", Q.LDS_SHAPES)
def test_lds_shapes_reach_both_loops(m, n):
    assert capi.load().lp_simplex_bounded_fits(m, n) == 1
    dual = primal = 0
    for mx in (True, False):
        for seed in Q.LDS_SEEDS:
            cold = Q.cold_ref(m, n, seed, mx)
            if cold["status"] != OPTIMAL:
                continue
            for kind in W.PERTURBATIONS:
                r = Q.ref(("lds", m, n, seed, mx, kind), Q.warm(m, n, seed, mx, kind, cold), mx, n - m)
                dual += r["status"] == OPTIMAL and r["iters"][0] > 0
                primal += r["status"] == OPTIMAL and r["iters"][1] > 0
    assert dual >= 1 and primal >= 1


def test_beyond_the_lds_fit_every_case_is_optimal():
    counts = {"bound": 0, "cost": 0, "rhs": 0}
    for m, n, seed in Q.BEYOND:
        assert capi.load().lp_simplex_bounded_fits(m, n) == int((m, n) == (67, 201))
        for mx in (True, False):
            cold = Q.cold_ref(m, n, seed, mx)
            assert cold["status"] == OPTIMAL
            for kind in W.PERTURBATIONS:
                start = Q.warm(m, n, seed, mx, kind, cold)
                r = Q.ref(("beyond", m, n, seed, mx, kind), start, mx, n - m)
                assert r["status"] == OPTIMAL
                if (m, n, seed, mx, kind) in Q.BEYOND_ITERS:
                    assert r["iters"] == Q.BEYOND_ITERS[(m, n, seed, mx, kind)]
                if (m, n) != (160, 320):
                    continue
                if kind == "bound":   # the dual loop, and a flag changed: a row was complemented
                    counts[kind] += r["iters"][0] > 0 and bool(np.any(r["at_upper"] != start[6]))
                elif kind == "cost":   # the primal loop with flips
                    counts[kind] += r["iters"][0] == 0 and r["iters"][1] > 0 and r["iters"][2] > 0
                else:
                    counts[kind] += r["iters"][0] > 0
    assert counts == {"bound": 15, "cost": 14, "rhs": 13}


@pytest.mark.parametrize("seed,maximize", Q.DUAL_INFEASIBLE)
def test_dual_infeasible_cases(seed, maximize):
    cold = Q.cold_ref(160, 320, seed, maximize)
    assert cold["status"] == OPTIMAL
    start = Q.warm(160, 320, seed, maximize, "bound", cold)
    r = Q.ref(("dual-infeasible", seed, maximize), start, maximize, 160)
    assert r["status"] == INFEASIBLE and not np.any(start[4] < start[3]) and 28 <= r["iters"][0] <= 214
    assert np.any(r["at_upper"] != start[6])
    if (seed, maximize) in Q.DUAL_INFEASIBLE_ITERS:
        assert r["iters"] == Q.DUAL_INFEASIBLE_ITERS[(seed, maximize)]


def test_other_outcomes_at_160x320():
    cases = Q.outcomes_160(Q.cold_ref(160, 320, 1, True))
    for name, start, status, max_iter in cases:
        r = Q.ref(("outcome", name), start, True, 160, max_iter=max_iter)
        assert r["status"] == status, name
    assert [st for _, _, st, _ in cases] == [INFEASIBLE, UNBOUNDED, SINGULAR, BAD_ARG, ITER_LIMIT]
    assert np.any(cases[0][1][4] < cases[0][1][3])


def test_iteration_limit_sweep():
    start = Q.warm(160, 320, 1, True, "bound", Q.cold_ref(160, 320, 1, True))
    for max_iter, status in Q.LIMIT_SWEEP.items():
        r = Q.ref(("limit", max_iter), start, True, 160, max_iter=max_iter)
        assert r["status"] == status and r["iters"] == [min(max_iter, 41), 0, 0]


def test_more_rows_than_selector_threads_in_order():
    # (the reversed basis takes the reference's crash at 1100 rows, seconds of host time: the GPU test computes it)
    m, n = Q.TALL_SHAPE
    assert m > 1024
    start = Q.tall(False)
    r = Q.ref(("tall", False), start, False, n - m, max_iter=Q.TALL_MAX_ITER)
    assert r["status"] == ITER_LIMIT and r["iters"] == Q.TALL_ITERS and int(r["at_upper"].sum()) == Q.TALL_FLAGS


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("maximize", [True, False])
def test_unit_basis_with_basic_costs(reverse, maximize):
    start = Q.unit_costs(1, reverse)
    A, c, basis = start[0], start[2], start[5]
    assert np.array_equal(A[:, np.sort(basis)], np.eye(160)) and np.all(c[basis] >= 0.1)
    r = Q.ref(("unit-costs", reverse, maximize), start, maximize, 160)
    assert r["status"] == OPTIMAL and r["iters"][0] == 0 and r["iters"][1] > 100
    if not reverse:
        assert r["iters"] == Q.UNIT_COST_ITERS[(1, maximize)]


@pytest.mark.parametrize("eps", [0.0, 1e-12])
def test_eps_zero_and_tiny_still_pivot(eps):
    start = Q.warm(67, 201, 1, True, "bound", Q.cold_ref(67, 201, 1, True))
    r = Q.ref(("eps", eps), start, True, 134, eps=eps, max_iter=2000)
    assert r["status"] in (OPTIMAL, INFEASIBLE, ITER_LIMIT) and r["iters"][0] > 0


@pytest.mark.parametrize("m,n", [(32, 96), (160, 320)])
@pytest.mark.parametrize("maximize", [True, False])
def test_identity_anchor_runs_both_loops(m, n, maximize):
    A, b, c, slack = capi.gen_lp(3, m, n)
    if not maximize:
        c = -c
    cold = resolve_ref.resolve(A, b, c, slack, maximize)
    assert cold["status"] == OPTIMAL
    lo, hi, up = np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32)
    b2 = resolve_ref.scale_rows(3, b)
    for bb, basis, which in ((b2, cold["basis"], 0), (b, slack, 1)):
        r = resolve_ref.resolve(A, bb, c, basis, maximize, n - m)
        w = W.resolve(A, bb, c, lo, hi, basis, up, maximize, n - m)
        assert r["status"] == w["status"] == OPTIMAL and tuple(r["iters"]) == tuple(w["iters"][:2])
        assert r["iters"][which] > 0 and np.array_equal(r["x"], w["x"]) and r["obj"] == w["obj"]
