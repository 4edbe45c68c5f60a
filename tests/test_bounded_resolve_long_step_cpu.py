"""The bound-flipping dual ratio test of the bounded re-solve without a GPU: tests/ref/bounded_resolve_long_step_ref.c
against the reference it restates (dual_ratio 0 is bounded_resolve_dual_rules_ref.c bit for bit on every branch), the
long-step test against the textbook one on status, optimum, feasibility and pivot count, the pinned counts and
iteration limits, the edge cases of the flip decision, the infeasible verdict's proof, what the tall case and the
multi-flip cases of the GPU tests reach, and what the new entries and the bindings do without a device."""
import ctypes as C
import inspect

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_resolve_dual_rules_ref as D
from tests import bounded_resolve_large_cases as Q
from tests import bounded_resolve_long_step_cases as Y
from tests import bounded_resolve_long_step_ref as L
from tests import bounded_resolve_ref as W
from tests.test_bounded_resolve_dual_rules_cpu import _identical

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def _large_case_starts():
    """(start, maximize, n_orig, max_iter) of every re-solve input of bounded_resolve_large_cases: the LDS shapes and
    BEYOND after each perturbation, the outcomes the perturbations do not reach, and the tall case under its cap."""
    shapes = [(m, n, seed) for m, n in Q.LDS_SHAPES for seed in Q.LDS_SEEDS] + Q.BEYOND
    for m, n, seed in shapes:
        for maximize in (True, False):
            cold = Q.cold_ref(m, n, seed, maximize)
            if cold["status"] != OPTIMAL:
                continue
            for kind in W.PERTURBATIONS:
                yield Q.warm(m, n, seed, maximize, kind, cold), maximize, n - m, 10000
    for _, start, _, max_iter in Q.outcomes_160(Q.cold_ref(160, 320, 1, True)):
        yield start, True, 160, max_iter
    for reverse in (False, True):
        yield Q.tall(reverse), False, Q.TALL_SHAPE[1] - Q.TALL_SHAPE[0], Q.TALL_MAX_ITER


@pytest.fixture(scope="module")
def starts():
    return list(_large_case_starts())


@pytest.fixture(scope="module")
def both(starts):
    """Per dual rule and start, the textbook and the long-step result with the full x (n_orig = n)."""
    out = {}
    for dual_rule in L.DUAL_RULES:
        out[dual_rule] = [(s, mx, L.resolve(*s, mx, None, max_iter=it, dual_rule=dual_rule, dual_ratio=L.TEXTBOOK),
                           L.resolve(*s, mx, None, max_iter=it, dual_rule=dual_rule, dual_ratio=L.LONG_STEP))
                          for s, mx, _, it in starts]
    return out


@pytest.mark.parametrize("dual_rule", L.DUAL_RULES)
def test_textbook_ratio_equals_the_dual_rules_reference(starts, dual_rule):
    ran = dual = 0
    for start, maximize, n_orig, max_iter in starts:
        old = D.resolve(*start, maximize, n_orig, max_iter=max_iter, dual_rule=dual_rule)
        _identical(L.resolve(*start, maximize, n_orig, max_iter=max_iter, dual_rule=dual_rule, dual_ratio=L.TEXTBOOK), old)
        ran += 1
        dual += old["iters"][0] > 0
    assert ran > 100 and dual > 30
    # under a primal rule too: the primal branch is the parent's under either ratio test
    start = Q.warm(160, 320, 1, True, "cost", Q.cold_ref(160, 320, 1, True))
    for rule in L.RULES:
        old = D.resolve(*start, True, 160, rule=rule, dual_rule=dual_rule)
        assert old["iters"][0] == 0 and old["iters"][1] > 0
        for ratio in (L.TEXTBOOK, L.LONG_STEP):
            _identical(L.resolve(*start, True, 160, rule=rule, dual_rule=dual_rule, dual_ratio=ratio), old)


@pytest.mark.parametrize("dual_rule", L.DUAL_RULES)
def test_long_step_against_textbook(both, dual_rule):
    flips_by_shape, pivots_text, pivots_long, optimal = {}, 0, 0, 0
    for start, maximize, a, g in both[dual_rule]:
        A, b, c, lo, hi, _, _ = start
        assert g["status"] == a["status"]
        if a["status"] == ITER_LIMIT:   # (a cap on the dual pivots cuts the two loops at different points)
            continue
        if a["iters"][0] == 0:
            _identical(g, a)   # the dual loop did not run, or found nothing to pivot on
            continue
        flips_by_shape[A.shape] = flips_by_shape.get(A.shape, 0) + (g["iters"][2] > 0)
        pivots_text += a["iters"][0]
        pivots_long += g["iters"][0]
        assert g["iters"][1] == 0
        if a["status"] != OPTIMAL:
            continue
        optimal += 1
        assert abs(g["obj"] - a["obj"]) <= 1e-9 * max(1.0, abs(a["obj"]))
        x = g["x"]
        # (a basic value passes the loop's test when it is within eps of its bound; lo + w adds a rounding of x's size)
        slack = 1e-9 + 4 * np.finfo(float).eps * np.maximum(1.0, np.abs(x))
        assert np.all(x >= lo - slack) and np.all(x <= hi + slack)
        assert np.abs(A @ x - b).max() <= 1e-7
    assert optimal >= 30
    assert all(count > 0 for count in flips_by_shape.values()) and len(flips_by_shape) >= 6
    assert pivots_long < pivots_text


def test_pinned_counts():
    for (m, n, seed, maximize, kind), (text, long) in Y.PINNED_ITERS.items():
        start = Y.warm(m, n, seed, maximize, kind)
        a = Y.ref(("pinned", m, n, seed, maximize, kind), start, maximize, n - m, dual_ratio=L.TEXTBOOK)
        g = Y.ref(("pinned", m, n, seed, maximize, kind), start, maximize, n - m)
        assert a["iters"] == text and g["iters"] == long and a["status"] == g["status"]
        assert a["status"] == (INFEASIBLE if seed == 22 else OPTIMAL)
    for key in ((160, 320, 1, True, "bound"),):
        assert Y.PINNED_ITERS[key][0] == Q.BEYOND_ITERS[key]


def test_iteration_limits():
    start = Y.warm(160, 320, 1, True, "bound")
    for max_iter, status in Y.LIMIT_SWEEP.items():
        r = Y.ref(("limit", max_iter), start, True, 160, max_iter=max_iter)
        assert r["status"] == status and r["iters"][:2] == [min(max_iter, Y.LIMIT_PIVOTS), 0]
    assert Y.ref(("limit", 28), start, True, 160, max_iter=28)["iters"] == Y.PINNED_ITERS[(160, 320, 1, True, "bound")][1]
    r = L.resolve(*start, True, 160, max_iter=0)
    assert r["status"] == ITER_LIMIT and r["iters"] == [0, 0, 0]


@pytest.mark.parametrize("kind", sorted(Y.EDGE_RESULTS))
@pytest.mark.parametrize("dual_rule", L.DUAL_RULES)
def test_edges_of_the_flip_decision(kind, dual_rule):
    start = Y.edge(kind)
    status, iters, flags = Y.EDGE_RESULTS[kind]
    r = L.resolve(*start, False, dual_rule=dual_rule)
    assert r["status"] == status and r["iters"] == iters and r["at_upper"][:3].tolist() == flags
    assert r["at_upper"][3:].tolist() == [0, 0]
    if kind == "fixed":      # x0 is fixed at 0, flipped and passed; x1 entered
        assert start[4][0] == 0.0 and r["x"][:3].tolist() == [0., 2., 0.] and r["obj"] == 4.0
    if kind == "unbounded":  # x0 went to its upper bound; x1, without one, entered
        assert np.isinf(start[4][1]) and r["x"][:3].tolist() == [1., 1., 0.] and r["obj"] == 3.0
    if kind == "cure":       # the textbook step
        assert r["x"][:3].tolist() == [2., 0., 0.]
        _identical(r, L.resolve(*start, False, dual_rule=dual_rule, dual_ratio=L.TEXTBOOK))
    if kind == "all":        # every candidate flipped, the row still violated: the basis stays, the flags say flipped
        assert np.array_equal(r["basis"], start[5]) and Y.held_row_proves_infeasible(start, r)
        assert L.resolve(*start, False, dual_rule=dual_rule, dual_ratio=L.TEXTBOOK)["status"] == INFEASIBLE


@pytest.mark.parametrize("dual_rule", L.DUAL_RULES)
def test_an_infeasible_verdict_returns_its_proof(both, dual_rule):
    seen = 0
    cases = [(s, mx, g) for s, mx, _, g in both[dual_rule]]
    for seed, maximize in Q.DUAL_INFEASIBLE:
        start = Y.warm(160, 320, seed, maximize, "bound")
        cases.append((start, maximize, Y.ref(("dual-infeasible", seed, maximize), start, maximize, 160, dual_rule=dual_rule)))
    for start, maximize, g in cases:
        if g["status"] != INFEASIBLE or np.any(start[4] < start[3]):
            continue
        assert Y.held_row_proves_infeasible(start, g)
        seen += g["iters"][2] > 0
    assert seen >= 4   # (verdicts reached after flips)


@pytest.mark.parametrize("dual_rule", L.DUAL_RULES)
def test_the_tall_case_flips_beyond_the_selectors_threads(dual_rule):
    start = Y.tall_boxed(False)
    A = start[0]
    m, n = A.shape
    assert (m, n) == Q.TALL_SHAPE and m > 1024
    steps = Y.steps(("tall", False), start, False, Y.TALL_MAX_ITER, dual_rule)
    assert len(steps) == Y.TALL_MAX_ITER   # still running at the cap
    assert any(s["flipped"] and s["complemented"] for s in steps)   # a flip on a row held complemented
    assert any(len(s["flipped"]) >= 2 for s in steps)               # the rescan more than once in one launch
    # a flipped column with an entry in a row beyond the first 1024: the flip's second stride moves that row's xB
    deep = False
    for s in steps:
        basis = np.asarray(start[5]) if s["before"] is None else s["before"]["basis"]
        for j in s["flipped"]:
            col = np.linalg.solve(A[:, basis], A[:, j])
            deep |= bool(np.any(np.abs(col[1024:]) > 1e-6))
    assert deep
    # from the reversed slack basis the crash and the row permutation run first, and the loop then does the same
    last = steps[-1]["after"]
    r = Y.ref(("tall", True), Y.tall_boxed(True), False, n - m, max_iter=Y.TALL_MAX_ITER, dual_rule=dual_rule)
    assert r["status"] == ITER_LIMIT and r["iters"] == last["iters"] and r["iters"][2] > 0
    assert np.array_equal(r["at_upper"], last["at_upper"]) and np.array_equal(r["basis"][::-1], last["basis"])


def test_some_case_of_every_set_flips_twice_in_one_iteration():
    # the LDS shapes' and the 160 x 320 starts of the GPU tests
    for key in [(32, 96, 1, True, "bound"), (64, 192, 1, False, "rhs"), (160, 320, 1, True, "bound")]:
        m, n, seed, maximize, kind = key
        steps = Y.steps(("multi",) + key, Y.warm(m, n, seed, maximize, kind), maximize, 8)
        assert any(len(s["flipped"]) >= 2 for s in steps), key


@pytest.mark.parametrize("dual_ratio", [2, -1])
def test_the_reference_refuses_an_unknown_dual_ratio_before_writing(dual_ratio):
    start = Y.edge("cure")
    r = L.resolve(*start, False, dual_ratio=dual_ratio)
    assert r["status"] == BAD_ARG and np.isnan(r["x"]).all() and np.isnan(r["obj"])
    assert np.all(r["basis"] == -1) and not r["at_upper"].any() and r["iters"] == [0, 0, 0]
    # (ahead of everything else: a bad dual rule, a bad pivot rule and a bad basis beside it change nothing)
    bad = np.full_like(start[5], -7)
    r = L.resolve(*start[:5], bad, start[6], False, rule=9, dual_rule=5, dual_ratio=dual_ratio)
    assert r["status"] == BAD_ARG and np.all(r["basis"] == -1)


def test_new_entries_refuse_a_null_context():
    lib = capi.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    A, b, c, lo, hi, basis, up = Y.edge("cure")
    m, n = A.shape
    Af = capi.colmajor(A)
    z, zi = np.zeros(n), np.zeros(n, np.int32)
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(dp)   # noqa: E731
    i = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(ip)   # noqa: E731
    for name in ("lp_simplex_bounded_resolve_ratio_ex", "lp_simplex_bounded_resolve_large_ratio_ex"):
        assert getattr(lib, name)(None, d(Af), m, n, d(b), d(c), d(lo), d(hi), i(basis), i(up), 0, n, 1e-9, 100, d(z),
                                  i(zi), i(zi), d(z), i(zi), 0, 0, 1) == BAD_ARG
    assert lib.lp_simplex_bounded_resolve_batched_ratio_ex(None, 1, d(Af), m, n, d(b), d(c), d(lo), d(hi), i(basis),
                                                           i(up), 0, n, 1e-9, 100, d(z), i(zi), i(zi), d(z), i(zi),
                                                           i(zi), 0, 0, 1) == BAD_ARG


def test_bindings():
    for name in ("bounded_resolve", "bounded_resolve_batched", "bounded_resolve_large"):
        p = inspect.signature(getattr(capi.Context, name)).parameters
        assert "dual_ratio" in p and p["dual_ratio"].default is None and p["dual_rule"].default is None
    assert capi.dual_ratio_id("textbook") == capi.DUAL_RATIO_TEXTBOOK == 0
    assert capi.dual_ratio_id("Long_Step") == capi.DUAL_RATIO_LONG_STEP == 1
    assert capi.dual_ratio_id(7) == 7 and capi.Context.dual_ratio_id("long_step") == 1
    with pytest.raises(ValueError):
        capi.dual_ratio_id("harris")
    for name in ("lp_simplex_bounded_resolve", "lp_simplex_bounded_resolve_batched", "lp_simplex_bounded_resolve_large"):
        assert capi.SIGNATURES[name + "_ratio_ex"][1] == capi.SIGNATURES[name + "_dual_ex"][1] + [C.c_int]
