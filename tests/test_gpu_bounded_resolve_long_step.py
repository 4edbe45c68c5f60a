"""The bound-flipping dual ratio test of the bounded re-solve on the GPU: lp_simplex_bounded_resolve_ratio_ex, its
_batched form and lp_simplex_bounded_resolve_large_ratio_ex.  Under LP_DUAL_RATIO_LONG_STEP status, x, obj, basis,
at_upper and the three counters equal tests/ref/bounded_resolve_long_step_ref.c's bit for bit under both dual rules: in
LDS, single and batched, after the "bound" and "rhs" perturbations, on the edges of the flip decision and at eps = 0;
on the tableau in HBM at the same shapes (where the LDS entry's result is the same), at an odd pitch, beyond the LDS
fit, from the dual loop's infeasible verdict, around the pinned pivot count and with more rows than the selector has
threads.  Under LP_DUAL_RATIO_TEXTBOOK every output is the _dual_ex entry's; a re-solve that takes the primal branch is
unchanged; an unknown dual ratio is refused with the outputs untouched.
tests/test_bounded_resolve_long_step_cpu.py shows on the reference that the inputs reach what is claimed here."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_resolve_large_cases as Q
from tests import bounded_resolve_long_step_cases as Y
from tests import bounded_resolve_long_step_ref as L
from tests.test_gpu_bounded import _row, _same
from tests.test_gpu_bounded_resolve_dual_rules import _stack, _warm_starts

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
LONG, TEXTBOOK = capi.DUAL_RATIO_LONG_STEP, capi.DUAL_RATIO_TEXTBOOK
DUAL_RULES = (capi.DUAL_DANTZIG, capi.DUAL_DEVEX)


@pytest.mark.parametrize("m,n", Q.LDS_SHAPES)
@pytest.mark.parametrize("maximize", [True, False])
@pytest.mark.parametrize("dual_rule", DUAL_RULES)
def test_lds_entries_after_bound_and_rhs_changes(ctx, m, n, maximize, dual_rule):
    cases = _warm_starts(m, n, maximize)
    assert len(cases) >= 2
    refs = [Y.ref(("lds",) + key, start, maximize, n - m, dual_rule=dual_rule) for key, start in cases]
    assert sum(r["iters"][0] > 0 for r in refs) >= 2
    batch = _stack([start for _, start in cases])
    out = ctx.bounded_resolve_batched(*batch, maximize, n - m, dual_rule=dual_rule, dual_ratio=LONG)
    plain = ctx.bounded_resolve_batched(*batch, maximize, n - m, dual_rule=dual_rule, dual_ratio=TEXTBOOK)
    old = ctx.bounded_resolve_batched(*batch, maximize, n - m, dual_rule=dual_rule)
    for k, ((_, start), r) in enumerate(zip(cases, refs)):
        _same(_row(out, k), r)
        _same(ctx.bounded_resolve(*start, maximize, n - m, dual_rule=dual_rule, dual_ratio=LONG), r)
        o = _row(old, k)
        o = dict(o, status=int(o["status"]), iters=[int(v) for v in o["iters"]])
        _same(_row(plain, k), o)
        _same(ctx.bounded_resolve(*start, maximize, n - m, dual_rule=dual_rule, dual_ratio=TEXTBOOK), o)
    if m > 6:
        assert sum(r["iters"][2] > 0 for r in refs) >= 1


@pytest.mark.parametrize("dual_rule", DUAL_RULES)
def test_every_entry_on_the_edges_of_the_flip_decision(ctx, dual_rule):
    kinds = sorted(Y.EDGE_RESULTS)
    starts = [Y.edge(kind) for kind in kinds]
    refs = [Y.ref(("edge", kind), s, False, dual_rule=dual_rule) for kind, s in zip(kinds, starts)]
    out = ctx.bounded_resolve_batched(*_stack(starts), False, dual_rule=dual_rule, dual_ratio=LONG)
    for k, (kind, start, r) in enumerate(zip(kinds, starts, refs)):
        assert (r["status"], r["iters"]) == Y.EDGE_RESULTS[kind][:2]
        _same(_row(out, k), r)
        _same(ctx.bounded_resolve(*start, False, dual_rule=dual_rule, dual_ratio=LONG), r)
        _same(ctx.bounded_resolve_large(*start, False, dual_rule=dual_rule, dual_ratio=LONG), r)


@pytest.mark.parametrize("dual_rule", DUAL_RULES)
def test_lds_batch_at_eps_zero(ctx, dual_rule):
    m, n = 32, 96
    cases = _warm_starts(m, n, True)
    out = ctx.bounded_resolve_batched(*_stack([s for _, s in cases]), True, n - m, eps=0.0, max_iter=2000,
                                      dual_rule=dual_rule, dual_ratio=LONG)
    flips = 0
    for k, (key, start) in enumerate(cases):
        r = Y.ref(("eps0",) + key, start, True, n - m, eps=0.0, max_iter=2000, dual_rule=dual_rule)
        _same(_row(out, k), r)
        _same(ctx.bounded_resolve_large(*start, True, n - m, eps=0.0, max_iter=2000, dual_rule=dual_rule, dual_ratio=LONG), r)
        flips += r["iters"][2]
    assert flips > 0


@pytest.mark.parametrize("m,n", Q.LDS_SHAPES)
@pytest.mark.parametrize("dual_rule", DUAL_RULES)
def test_hbm_entry_at_shapes_that_also_fit_lds(ctx, m, n, dual_rule):
    ran = 0
    for maximize in (True, False):
        for key, start in _warm_starts(m, n, maximize):
            r = Y.ref(("lds",) + key, start, maximize, n - m, dual_rule=dual_rule)
            g = ctx.bounded_resolve_large(*start, maximize, n - m, dual_rule=dual_rule, dual_ratio=LONG)
            _same(g, r)
            _same(g, ctx.bounded_resolve(*start, maximize, n - m, dual_rule=dual_rule, dual_ratio=LONG))
            _same(ctx.bounded_resolve_large(*start, maximize, n - m, dual_rule=dual_rule, dual_ratio=TEXTBOOK),
                  ctx.bounded_resolve_large(*start, maximize, n - m, dual_rule=dual_rule))
            ran += r["iters"][0] > 0
    assert ran >= 3


@pytest.mark.parametrize("m,n,seeds", [(67, 201, (1, 2)), (160, 320, (1, 2, 3))])
@pytest.mark.parametrize("dual_rule", DUAL_RULES)
def test_hbm_entry_beyond_the_lds_shapes(ctx, m, n, seeds, dual_rule):
    dual = flips = 0
    for seed in seeds:
        for maximize in (True, False):
            cold = Q.cold_ref(m, n, seed, maximize)
            assert cold["status"] == OPTIMAL
            for kind in ("bound", "rhs"):
                key = (m, n, seed, maximize, kind)
                start = Q.warm(m, n, seed, maximize, kind, cold)
                r = Y.ref(("beyond",) + key, start, maximize, n - m, dual_rule=dual_rule)
                assert r["status"] == OPTIMAL
                if key in Y.PINNED_ITERS and dual_rule == capi.DUAL_DANTZIG:
                    assert r["iters"] == Y.PINNED_ITERS[key][1]
                _same(ctx.bounded_resolve_large(*start, maximize, n - m, dual_rule=dual_rule, dual_ratio=LONG), r)
                dual += r["iters"][0] > 0
                flips += r["iters"][2] > 0
    assert dual >= 4 and flips >= 2
    start = Y.warm(m, n, 1, True, "bound")
    _same(ctx.bounded_resolve_large(*start, True, n - m, dual_rule=dual_rule, dual_ratio=TEXTBOOK),
          ctx.bounded_resolve_large(*start, True, n - m, dual_rule=dual_rule))


@pytest.mark.parametrize("seed,maximize", Q.DUAL_INFEASIBLE)
def test_hbm_entry_infeasible_from_the_dual_loop(ctx, seed, maximize):
    m, n = 160, 320
    start = Y.warm(m, n, seed, maximize, "bound")
    for dual_rule in DUAL_RULES:
        r = Y.ref(("dual-infeasible", seed, maximize), start, maximize, n - m, dual_rule=dual_rule)
        assert r["status"] == INFEASIBLE and not np.any(start[4] < start[3]) and r["iters"][2] > 0
        g = ctx.bounded_resolve_large(*start, maximize, n - m, dual_rule=dual_rule, dual_ratio=LONG)
        _same(g, r)
        assert np.any(g["at_upper"] != start[6])


def test_hbm_entry_iteration_limits(ctx):
    start = Y.warm(160, 320, 1, True, "bound")
    for max_iter, status in Y.LIMIT_SWEEP.items():
        r = Y.ref(("limit", max_iter), start, True, 160, max_iter=max_iter)
        assert r["status"] == status
        _same(ctx.bounded_resolve_large(*start, True, 160, max_iter=max_iter, dual_ratio=LONG), r)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dual_rule", DUAL_RULES)
def test_hbm_entry_with_more_rows_than_selector_threads(ctx, reverse, dual_rule):
    m, n = Q.TALL_SHAPE
    start = Y.tall_boxed(reverse)
    r = Y.ref(("tall", reverse), start, False, n - m, max_iter=Y.TALL_MAX_ITER, dual_rule=dual_rule)
    assert r["status"] == ITER_LIMIT and r["iters"][0] == Y.TALL_MAX_ITER and r["iters"][2] > Y.TALL_MAX_ITER
    _same(ctx.bounded_resolve_large(*start, False, n - m, max_iter=Y.TALL_MAX_ITER, dual_rule=dual_rule, dual_ratio=LONG), r)


@pytest.mark.parametrize("pivot_rule", L.RULES)
def test_primal_branch_is_untouched(ctx, pivot_rule):
    ran = 0
    for m, n in [(32, 96), (160, 320)]:
        start = Y.warm(m, n, 1, True, "cost")
        old = ctx.bounded_resolve_large(*start, True, n - m, pivot_rule=pivot_rule)
        assert old["status"] == OPTIMAL and old["iters"][0] == 0
        ran += old["iters"][1] + old["iters"][2] > 0
        _same(old, L.resolve(*start, True, n - m, rule=pivot_rule, dual_rule=L.DUAL_DEVEX, dual_ratio=L.LONG_STEP))
        for dual_rule in DUAL_RULES:
            for ratio in (TEXTBOOK, LONG):
                kw = dict(pivot_rule=pivot_rule, dual_rule=dual_rule, dual_ratio=ratio)
                _same(ctx.bounded_resolve_large(*start, True, n - m, **kw), old)
                if m == 32:
                    _same(ctx.bounded_resolve(*start, True, n - m, **kw), old)
                    _same(_row(ctx.bounded_resolve_batched(*_stack([start]), True, n - m, **kw), 0), old)
    assert ran >= 1


def test_refusals(ctx):
    m, n = 32, 96
    start = Y.warm(m, n, 1, True, "bound")
    for entry in (ctx.bounded_resolve, ctx.bounded_resolve_large):
        for bad in (2, -1):
            with pytest.raises(capi.LPError) as e:
                entry(*start, True, n - m, dual_ratio=bad)
            assert e.value.code == BAD_ARG
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_resolve_batched(*_stack([start]), True, n - m, dual_ratio=2)
    assert e.value.code == BAD_ARG
    # the outputs of a refused call are untouched
    A, b, c, lo, hi, basis, up = start
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    Af = capi.colmajor(A)
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(dp)   # noqa: E731
    i = lambda a: a.ctypes.data_as(ip)   # noqa: E731
    bi, ui = np.ascontiguousarray(basis, np.int32), np.ascontiguousarray(up, np.int32)
    for name in ("lp_simplex_bounded_resolve_ratio_ex", "lp_simplex_bounded_resolve_large_ratio_ex",
                 "lp_simplex_bounded_resolve_batched_ratio_ex"):
        x, obj = np.full(n, 7.5), np.full(1, 7.5)
        bo, uo, it, st = (np.full(k, 77, np.int32) for k in (m, n, 3, 1))
        head = (ctx.h, 1) if "batched" in name else (ctx.h,)
        tail = (i(st), 0, 0, 2) if "batched" in name else (0, 0, 2)
        rc = getattr(ctx.lib, name)(*head, d(Af), m, n, d(b), d(c), d(lo), d(hi), i(bi), i(ui), 1, n, 1e-9, 100, d(x),
                                    i(bo), i(uo), d(obj), i(it), *tail)
        assert rc == BAD_ARG
        assert np.all(x == 7.5) and obj[0] == 7.5
        assert all(np.all(a == 77) for a in (bo, uo, it, st))
    # a shape beyond the LDS fit is refused by the LDS entries under either ratio test
    big = Y.warm(160, 320, 1, True, "bound")
    for ratio in (TEXTBOOK, LONG):
        with pytest.raises(capi.LPError) as e:
            ctx.bounded_resolve(*big, True, 160, dual_ratio=ratio)
        assert e.value.code == BAD_ARG
    # the context still works
    _same(ctx.bounded_resolve(*start, True, n - m, dual_ratio=LONG), Y.ref(("lds", m, n, 1, True, "bound"), start, True, n - m))
    _same(ctx.bounded_resolve_large(*big, True, 160, dual_ratio=LONG), Y.ref(("beyond", 160, 320, 1, True, "bound"), big, True, 160))
