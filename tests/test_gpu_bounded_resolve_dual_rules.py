"""The dual pricing rule of the bounded re-solve on the GPU: lp_simplex_bounded_resolve_dual_ex, its _batched form and
lp_simplex_bounded_resolve_large_dual_ex.  Under LP_DUAL_DEVEX status, x, obj, basis, at_upper and the three counters
equal tests/ref/bounded_resolve_dual_rules_ref.c's bit for bit: in LDS, single and batched, after the "bound" and "rhs"
perturbations, on the outcomes of the dual loop, on an exact tie across a wave seam and at eps = 0; on the tableau in
HBM at the same shapes (where the LDS entry's result is the same), beyond the LDS fit, from the dual loop's infeasible
verdict, with more rows than the selector has threads and on an exact tie across its 1024-thread seam.  Under
LP_DUAL_DANTZIG every output is the _ex entry's; a re-solve that takes the primal branch is the _ex entry's under
either dual rule; an unknown dual rule is refused with the outputs untouched.
tests/test_bounded_resolve_dual_rules_cpu.py shows on the reference that the inputs reach what is claimed here."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_resolve_dual_rules_cases as X
from tests import bounded_resolve_dual_rules_ref as D
from tests import bounded_resolve_large_cases as Q
from tests import bounded_resolve_ref as W
from tests.test_gpu_bounded import _row, _same

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
DEVEX, DANTZIG = capi.DUAL_DEVEX, capi.DUAL_DANTZIG


def _warm_starts(m, n, maximize, kinds=("bound", "rhs")):
    """[(key, start)] of the LDS shape's warm starts of seeds 1-3 whose cold solve was optimal."""
    out = []
    for seed in Q.LDS_SEEDS:
        cold = Q.cold_ref(m, n, seed, maximize)
        if cold["status"] != OPTIMAL:
            continue
        out += [((m, n, seed, maximize, kind), Q.warm(m, n, seed, maximize, kind, cold)) for kind in kinds]
    return out


def _stack(starts):
    return [np.stack([s[i] for s in starts]) for i in range(7)]


@pytest.mark.parametrize("m,n", Q.LDS_SHAPES)
@pytest.mark.parametrize("maximize", [True, False])
def test_lds_entries_after_bound_and_rhs_changes(ctx, m, n, maximize):
    cases = _warm_starts(m, n, maximize)
    assert len(cases) >= 2
    refs = [X.ref(("lds",) + key, start, maximize, n - m) for key, start in cases]
    assert sum(r["iters"][0] > 0 for r in refs) >= 2
    batch = _stack([start for _, start in cases])
    out = ctx.bounded_resolve_batched(*batch, maximize, n - m, dual_rule=DEVEX)
    plain = ctx.bounded_resolve_batched(*batch, maximize, n - m, dual_rule=DANTZIG)
    old = ctx.bounded_resolve_batched(*batch, maximize, n - m, pivot_rule=capi.PIVOT_DANTZIG)
    for k, ((_, start), r) in enumerate(zip(cases, refs)):
        _same(_row(out, k), r)
        _same(ctx.bounded_resolve(*start, maximize, n - m, dual_rule=DEVEX), r)
        o = _row(old, k)
        o = dict(o, status=int(o["status"]), iters=[int(v) for v in o["iters"]])
        _same(_row(plain, k), o)
        _same(ctx.bounded_resolve(*start, maximize, n - m, dual_rule=DANTZIG), o)


def test_lds_entries_on_the_dual_loops_outcomes(ctx):
    max_iter = 3
    cases = [(name, start) for name, start, _ in W.outcome_cases(max_iter=max_iter)
             if name in ("dual_complement", "dual_infeasible", "iter_limit")]
    assert len(cases) == 3
    refs = [X.ref(("outcome", name), start, True, max_iter=max_iter) for name, start in cases]
    assert all(r["iters"][0] > 0 or r["status"] == INFEASIBLE for r in refs)
    out = ctx.bounded_resolve_batched(*_stack([s for _, s in cases]), True, max_iter=max_iter, dual_rule=DEVEX)
    for k, ((name, start), r) in enumerate(zip(cases, refs)):
        _same(_row(out, k), r)
        _same(ctx.bounded_resolve(*start, True, max_iter=max_iter, dual_rule=DEVEX), r)
        _same(ctx.bounded_resolve_large(*start, True, max_iter=max_iter, dual_rule=DEVEX), r)
        o = ctx.bounded_resolve(*start, True, max_iter=max_iter, pivot_rule=capi.PIVOT_DANTZIG)
        _same(ctx.bounded_resolve(*start, True, max_iter=max_iter, dual_rule=DANTZIG), o)


@pytest.mark.parametrize("max_iter", [1, 20])
def test_lds_entries_on_a_tie_across_the_wave_seam(ctx, max_iter):
    m, n, p = X.TIE_SMALL
    assert ctx.bounded_dual_rule_fits(m, n, "dantzig", "devex")
    start = X.tie(m, n, p)
    r = X.ref(("tie", m, n, p, max_iter), start, False, max_iter=max_iter)
    if max_iter == 1:
        assert X.left_at(start, r) == [p]
    g = ctx.bounded_resolve(*start, False, max_iter=max_iter, dual_rule=DEVEX)
    _same(g, r)
    out = ctx.bounded_resolve_batched(*_stack([start, start]), False, max_iter=max_iter, dual_rule=DEVEX)
    _same(_row(out, 0), r)
    _same(_row(out, 1), r)
    _same(ctx.bounded_resolve_large(*start, False, max_iter=max_iter, dual_rule=DEVEX), r)


def test_lds_batch_at_eps_zero(ctx):
    m, n = 32, 96
    cases = _warm_starts(m, n, True)
    out = ctx.bounded_resolve_batched(*_stack([s for _, s in cases]), True, n - m, eps=0.0, max_iter=2000, dual_rule=DEVEX)
    for k, (key, start) in enumerate(cases):
        r = X.ref(("eps0",) + key, start, True, n - m, eps=0.0, max_iter=2000)
        _same(_row(out, k), r)
        _same(ctx.bounded_resolve_large(*start, True, n - m, eps=0.0, max_iter=2000, dual_rule=DEVEX), r)


@pytest.mark.parametrize("m,n", Q.LDS_SHAPES)
def test_hbm_entry_at_shapes_that_also_fit_lds(ctx, m, n):
    ran = 0
    for maximize in (True, False):
        for key, start in _warm_starts(m, n, maximize):
            r = X.ref(("lds",) + key, start, maximize, n - m)
            g = ctx.bounded_resolve_large(*start, maximize, n - m, dual_rule=DEVEX)
            _same(g, r)
            _same(g, ctx.bounded_resolve(*start, maximize, n - m, dual_rule=DEVEX))
            _same(ctx.bounded_resolve_large(*start, maximize, n - m, dual_rule=DANTZIG),
                  ctx.bounded_resolve_large(*start, maximize, n - m, pivot_rule=capi.PIVOT_DANTZIG))
            ran += r["iters"][0] > 0
    assert ran >= 3


@pytest.mark.parametrize("m,n,seeds", [(67, 201, (1, 2)), (160, 320, (1, 2, 3))])
def test_hbm_entry_beyond_the_lds_shapes(ctx, m, n, seeds):
    dual = 0
    for seed in seeds:
        for maximize in (True, False):
            cold = Q.cold_ref(m, n, seed, maximize)
            assert cold["status"] == OPTIMAL
            for kind in ("bound", "rhs"):
                start = Q.warm(m, n, seed, maximize, kind, cold)
                r = X.ref(("beyond", m, n, seed, maximize, kind), start, maximize, n - m)
                assert r["status"] == OPTIMAL
                if (m, n, seed, maximize, kind) in X.DEVEX_ITERS:
                    assert r["iters"] == X.DEVEX_ITERS[(m, n, seed, maximize, kind)]
                _same(ctx.bounded_resolve_large(*start, maximize, n - m, dual_rule=DEVEX), r)
                dual += r["iters"][0] > 0
    assert dual >= 4
    start = Q.warm(m, n, 1, True, "bound", Q.cold_ref(m, n, 1, True))
    _same(ctx.bounded_resolve_large(*start, True, n - m, dual_rule=DANTZIG),
          ctx.bounded_resolve_large(*start, True, n - m, pivot_rule=capi.PIVOT_DANTZIG))


@pytest.mark.parametrize("seed", [20, 22])
def test_hbm_entry_infeasible_from_the_dual_loop(ctx, seed):
    m, n = 160, 320
    start = X.warm_160(seed, True, "bound")
    r = X.ref(("dual-infeasible", seed), start, True, n - m)
    assert r["status"] == INFEASIBLE and not np.any(start[4] < start[3]) and r["iters"][0] > 0
    g = ctx.bounded_resolve_large(*start, True, n - m, dual_rule=DEVEX)
    _same(g, r)
    assert np.any(g["at_upper"] != start[6])


def test_hbm_entry_iteration_limits(ctx):
    start = X.warm_160(1, True, "bound")
    for max_iter, status in X.DEVEX_LIMIT_SWEEP.items():
        r = X.ref(("limit", max_iter), start, True, 160, max_iter=max_iter)
        assert r["status"] == status
        _same(ctx.bounded_resolve_large(*start, True, 160, max_iter=max_iter, dual_rule=DEVEX), r)


@pytest.mark.parametrize("reverse", [False, True])
def test_hbm_entry_with_more_rows_than_selector_threads(ctx, reverse):
    m, n = Q.TALL_SHAPE
    start = Q.tall(reverse)
    r = X.ref(("tall", reverse), start, False, n - m, max_iter=Q.TALL_MAX_ITER)
    assert r["status"] == ITER_LIMIT and r["iters"] == X.TALL_DEVEX_ITERS
    assert int(r["at_upper"].sum()) == X.TALL_DEVEX_FLAGS
    _same(ctx.bounded_resolve_large(*start, False, n - m, max_iter=Q.TALL_MAX_ITER, dual_rule=DEVEX), r)


@pytest.mark.parametrize("max_iter", [1, 20])
def test_hbm_entry_on_a_tie_across_the_thread_seam(ctx, max_iter):
    m, n, p = X.TIE_LARGE
    start = X.tie(m, n, p)
    r = X.ref(("tie", m, n, p, max_iter), start, False, max_iter=max_iter)
    assert r["iters"] == [max_iter, 0, 0]
    if max_iter == 1:
        assert X.left_at(start, r) == [p]
    _same(ctx.bounded_resolve_large(*start, False, max_iter=max_iter, dual_rule=DEVEX), r)


@pytest.mark.parametrize("pivot_rule", D.RULES)
def test_primal_branch_is_untouched(ctx, pivot_rule):
    ran = 0
    for m, n in [(32, 96), (160, 320)]:
        cold = Q.cold_ref(m, n, 1, True)
        start = Q.warm(m, n, 1, True, "cost", cold)
        old = ctx.bounded_resolve_large(*start, True, n - m, pivot_rule=pivot_rule)
        assert old["status"] == OPTIMAL and old["iters"][0] == 0
        ran += old["iters"][1] + old["iters"][2] > 0
        _same(old, D.resolve(*start, True, n - m, rule=pivot_rule, dual_rule=D.DUAL_DEVEX))
        for dual_rule in (DANTZIG, DEVEX):
            _same(ctx.bounded_resolve_large(*start, True, n - m, pivot_rule=pivot_rule, dual_rule=dual_rule), old)
            if m == 32:
                _same(ctx.bounded_resolve(*start, True, n - m, pivot_rule=pivot_rule, dual_rule=dual_rule), old)
                out = ctx.bounded_resolve_batched(*_stack([start]), True, n - m, pivot_rule=pivot_rule, dual_rule=dual_rule)
                _same(_row(out, 0), old)
    assert ran >= 1


def test_refusals(ctx):
    m, n = 32, 96
    start = Q.warm(m, n, 1, True, "bound", Q.cold_ref(m, n, 1, True))
    for entry in (ctx.bounded_resolve, ctx.bounded_resolve_large):
        for bad in (2, -1):
            with pytest.raises(capi.LPError) as e:
                entry(*start, True, n - m, dual_rule=bad)
            assert e.value.code == BAD_ARG
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_resolve_batched(*_stack([start]), True, n - m, dual_rule=2)
    assert e.value.code == BAD_ARG
    # the outputs of a refused call are untouched
    A, b, c, lo, hi, basis, up = start
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    Af = capi.colmajor(A)
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(dp)   # noqa: E731
    i = lambda a: a.ctypes.data_as(ip)   # noqa: E731
    bi, ui = np.ascontiguousarray(basis, np.int32), np.ascontiguousarray(up, np.int32)
    for name in ("lp_simplex_bounded_resolve_dual_ex", "lp_simplex_bounded_resolve_large_dual_ex",
                 "lp_simplex_bounded_resolve_batched_dual_ex"):
        x, obj = np.full(n, 7.5), np.full(1, 7.5)
        bo, uo, it, st = (np.full(k, 77, np.int32) for k in (m, n, 3, 1))
        head = (ctx.h, 1) if "batched" in name else (ctx.h,)
        tail = (i(st), 0, 2) if "batched" in name else (0, 2)
        rc = getattr(ctx.lib, name)(*head, d(Af), m, n, d(b), d(c), d(lo), d(hi), i(bi), i(ui), 1, n, 1e-9, 100, d(x),
                                    i(bo), i(uo), d(obj), i(it), *tail)
        assert rc == BAD_ARG
        assert np.all(x == 7.5) and obj[0] == 7.5
        assert all(np.all(a == 77) for a in (bo, uo, it, st))
    # a shape beyond the fit, and one that fits plain but not with m more doubles: the LDS entries refuse both
    assert not ctx.bounded_dual_rule_fits(160, 320, "dantzig", "devex")
    big = X.warm_160(1, True, "bound")
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_resolve(*big, True, 160, dual_rule=DEVEX)
    assert e.value.code == BAD_ARG
    wide = max(k for k in range(64, 400) if ctx.bounded_fits(64, k))
    assert not ctx.bounded_dual_rule_fits(64, wide, "dantzig", "devex")
    edge = X.tie(64, wide, 10)
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_resolve(*edge, False, max_iter=5, dual_rule=DEVEX)
    assert e.value.code == BAD_ARG
    _same(ctx.bounded_resolve(*edge, False, max_iter=5, dual_rule=DANTZIG),
          D.resolve(*edge, False, max_iter=5, dual_rule=D.DUAL_DANTZIG))
    _same(ctx.bounded_resolve_large(*edge, False, max_iter=5, dual_rule=DEVEX), D.resolve(*edge, False, max_iter=5, dual_rule=D.DUAL_DEVEX))
    # the context still works
    _same(ctx.bounded_resolve(*start, True, n - m, dual_rule=DEVEX), X.ref(("lds", m, n, 1, True, "bound"), start, True, n - m))
    _same(ctx.bounded_resolve_large(*big, True, 160, dual_rule=DEVEX), X.ref(("beyond", 160, 320, 1, True, "bound"), big, True, 160))
