"""lp_simplex_bounded_resolve_large on the GPU: the bounded-variable re-solve from a basis on the tableau in HBM.  Status,
x, obj, basis, at_upper and the three counters equal tests/ref/bounded_resolve_ref.c's bit for bit: at shapes that also
fit LDS (where the result is lp_simplex_bounded_resolve's too), beyond that fit after each perturbation of a cold
lp_simplex_bounded_large solve (an odd row length, the dual loop with complemented rows, the primal loop with flips),
LP_INFEASIBLE from the dual loop with the flag it toggled first, every other outcome, iteration limits among dual
pivots, more rows than the selectors have threads with and without the crash, a unit basis with costs to price out,
eps = 0; with lo = 0 and hi = inf the result is lp_simplex_resolve's; and the refusals.
tests/test_bounded_resolve_large_cpu.py shows on the reference that every input reaches what is claimed here."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_large_cases as K
from tests import bounded_resolve_large_cases as Q
from tests import bounded_resolve_ref as W
from tests import resolve_ref
from tests.test_gpu_bounded import _bits_equal, _same

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def _run(ctx, start, maximize, n_orig=None, **kw):
    """bounded_resolve_large, with a refusal (the binding raises) in the form of the reference's BAD_ARG result: the
    status, NaN for x and obj, zero counters and the given basis and flags."""
    try:
        return ctx.bounded_resolve_large(*start, maximize, n_orig, **kw)
    except capi.LPError as e:
        m, n = start[0].shape
        k = n if n_orig is None else n_orig
        return dict(status=e.code, x=np.full(k, np.nan), basis=np.asarray(start[5]), at_upper=np.asarray(start[6]),
                    obj=np.nan, iters=[0, 0, 0])


@pytest.mark.parametrize("m,n", Q.LDS_SHAPES)
@pytest.mark.parametrize("maximize", [True, False])
def test_shapes_that_also_fit_lds(ctx, m, n, maximize):
    ran = 0
    for seed in Q.LDS_SEEDS:
        A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, maximize)
        cold = ctx.bounded(A, b, c, lo, hi, maximize)
        _same(cold, Q.cold_ref(m, n, seed, maximize))
        if cold["status"] != OPTIMAL:
            continue
        for kind in W.PERTURBATIONS:
            start = Q.warm(m, n, seed, maximize, kind, cold)
            r = Q.ref(("lds", m, n, seed, maximize, kind), start, maximize, n - m)
            g = _run(ctx, start, maximize, n - m)
            _same(g, r)
            if r["status"] == BAD_ARG:   # neither primal nor dual feasible: both entries refuse
                with pytest.raises(capi.LPError):
                    ctx.bounded_resolve(*start, maximize, n - m)
                continue
            _same(g, ctx.bounded_resolve(*start, maximize, n - m))
            ran += 1
    assert ran >= 3


@pytest.mark.parametrize("m,n", sorted({(m, n) for m, n, _ in Q.BEYOND}))
def test_beyond_the_lds_fit(ctx, m, n):
    assert ctx.bounded_fits(m, n) == ((m, n) == (67, 201))
    dual = primal = flagged = flipped = 0
    for seed in [s for mm, nn, s in Q.BEYOND if (mm, nn) == (m, n)]:
        for maximize in (True, False):
            A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, maximize)
            cold = ctx.bounded_large(A, b, c, lo, hi, maximize)
            _same(cold, Q.cold_ref(m, n, seed, maximize))
            assert cold["status"] == OPTIMAL
            for kind in W.PERTURBATIONS:
                start = Q.warm(m, n, seed, maximize, kind, cold)
                r = Q.ref(("beyond", m, n, seed, maximize, kind), start, maximize, n - m)
                assert r["status"] == OPTIMAL
                _same(ctx.bounded_resolve_large(*start, maximize, n - m), r)
                if (m, n, seed, maximize, kind) in Q.BEYOND_ITERS:
                    assert r["iters"] == Q.BEYOND_ITERS[(m, n, seed, maximize, kind)]
                dual += r["iters"][0] > 0
                primal += r["iters"][1] > 0
                flagged += r["iters"][0] > 0 and bool(np.any(r["at_upper"] != start[6]))
                flipped += r["iters"][2] > 0
    assert dual >= 1 and primal >= 1 and flagged >= 1 and flipped >= 1   # a case of each kind ran


@pytest.mark.parametrize("seed,maximize", Q.DUAL_INFEASIBLE)
def test_infeasible_from_the_dual_loop(ctx, seed, maximize):
    m, n = 160, 320
    A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, maximize)
    cold = ctx.bounded_large(A, b, c, lo, hi, maximize)
    assert cold["status"] == OPTIMAL
    start = Q.warm(m, n, seed, maximize, "bound", cold)
    r = Q.ref(("dual-infeasible", seed, maximize), start, maximize, n - m)
    assert r["status"] == INFEASIBLE and not np.any(start[4] < start[3]) and 28 <= r["iters"][0] <= 214
    if (seed, maximize) in Q.DUAL_INFEASIBLE_ITERS:
        assert r["iters"] == Q.DUAL_INFEASIBLE_ITERS[(seed, maximize)]
    g = ctx.bounded_resolve_large(*start, maximize, n - m)
    _same(g, r)
    assert np.array_equal(g["at_upper"], r["at_upper"]) and np.any(g["at_upper"] != start[6])


def test_other_outcomes_at_160x320(ctx):
    m, n = 160, 320
    A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", 1, True)
    cold = ctx.bounded_large(A, b, c, lo, hi, True)
    assert cold["status"] == OPTIMAL
    cases = Q.outcomes_160(cold)
    assert [name for name, _, _, _ in cases] == ["crossed", "unbounded", "singular", "no_valid_start", "iter_limit"]
    for name, start, status, max_iter in cases:
        r = Q.ref(("outcome", name), start, True, n - m, max_iter=max_iter)
        assert r["status"] == status, name
        g = _run(ctx, start, True, n - m, max_iter=max_iter)
        _same(g, r)
        if name in ("crossed", "singular"):   # the given basis and flags come back
            assert np.array_equal(g["basis"], start[5]) and np.array_equal(g["at_upper"], start[6])
            assert g["iters"] == [0, 0, 0]


def test_outcomes_at_6x16(ctx):
    max_iter = 3
    for name, start, status in W.outcome_cases(max_iter=max_iter):
        r = W.resolve(*start, True, max_iter=max_iter)
        assert r["status"] == status, name
        _same(_run(ctx, start, True, max_iter=max_iter), r)


def test_iteration_limits_among_dual_pivots(ctx):
    m, n = 160, 320
    start = Q.warm(m, n, 1, True, "bound", Q.cold_ref(m, n, 1, True))
    for max_iter, status in Q.LIMIT_SWEEP.items():
        r = Q.ref(("limit", max_iter), start, True, n - m, max_iter=max_iter)
        assert r["status"] == status and r["iters"] == [min(max_iter, 41), 0, 0]
        _same(ctx.bounded_resolve_large(*start, True, n - m, max_iter=max_iter), r)


@pytest.mark.parametrize("reverse", [False, True])
def test_more_rows_than_selector_threads(ctx, reverse):
    m, n = Q.TALL_SHAPE
    start = Q.tall(reverse)
    r = Q.ref(("tall", reverse), start, False, n - m, max_iter=Q.TALL_MAX_ITER)
    assert r["status"] == ITER_LIMIT and r["iters"] == Q.TALL_ITERS and int(r["at_upper"].sum()) == Q.TALL_FLAGS
    _same(ctx.bounded_resolve_large(*start, False, n - m, max_iter=Q.TALL_MAX_ITER), r)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("maximize", [True, False])
def test_unit_basis_with_basic_costs(ctx, reverse, maximize):
    start = Q.unit_costs(1, reverse)
    r = Q.ref(("unit-costs", reverse, maximize), start, maximize, 160)
    assert r["status"] == OPTIMAL and r["iters"][0] == 0 and r["iters"][1] > 100
    if not reverse:
        assert r["iters"] == Q.UNIT_COST_ITERS[(1, maximize)]
    _same(ctx.bounded_resolve_large(*start, maximize, 160), r)


@pytest.mark.parametrize("eps", [0.0, 1e-12])
def test_eps_zero_and_tiny(ctx, eps):
    m, n = 67, 201
    start = Q.warm(m, n, 1, True, "bound", Q.cold_ref(m, n, 1, True))
    r = Q.ref(("eps", eps), start, True, n - m, eps=eps, max_iter=2000)
    _same(ctx.bounded_resolve_large(*start, True, n - m, eps=eps, max_iter=2000), r)


@pytest.mark.parametrize("m,n", [(32, 96), (160, 320)])
@pytest.mark.parametrize("maximize", [True, False])
def test_identity_anchor_equals_resolve(ctx, m, n, maximize):
    A, b, c, slack = capi.gen_lp(3, m, n)
    if not maximize:
        c = -c
    cold = ctx.simplex_solve(A, b, c, slack, maximize)
    assert cold["status"] == OPTIMAL
    b2 = resolve_ref.scale_rows(3, b)
    lo, hi, up = np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32)
    seen = []
    for bb, basis in ((b2, cold["basis"]), (b, slack)):   # the dual loop; the primal loop from the slack identity
        g = ctx.bounded_resolve_large(A, bb, c, lo, hi, basis, up, maximize, n - m)
        t = ctx.simplex_resolve(A, bb, c, basis, maximize, n - m)
        r = resolve_ref.resolve(A, bb, c, basis, maximize, n - m)
        assert g["status"] == t["status"] == r["status"] == OPTIMAL
        assert tuple(g["iters"][:2]) == tuple(t["iters"]) == tuple(r["iters"]) and g["iters"][2] == 0
        assert np.array_equal(g["basis"], t["basis"]) and np.array_equal(g["basis"], r["basis"])
        assert not g["at_upper"].any()
        for other in (t, r):
            _bits_equal(g["x"], other["x"])
            _bits_equal(g["obj"], other["obj"])
        seen.append(tuple(g["iters"]))
    assert seen[0][0] > 0 and seen[1][1] > 0


def test_refusals(ctx):
    m, n = 160, 320
    A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", 1, True)
    cold = Q.cold_ref(m, n, 1, True)
    basis, up = cold["basis"], cold["at_upper"]

    def refused(basis2, up2, lo2=lo, hi2=hi, eps=1e-9):
        if eps >= 0:
            assert W.resolve(A, b, c, lo2, hi2, basis2, up2, True)["status"] == BAD_ARG
        with pytest.raises(capi.LPError) as e:
            ctx.bounded_resolve_large(A, b, c, lo2, hi2, basis2, up2, True, eps=eps)
        assert e.value.code == BAD_ARG

    for bad_lo in (-np.inf, np.nan):
        lo2 = lo.copy()
        lo2[2] = bad_lo
        refused(basis, up, lo2=lo2)
    hi2 = hi.copy()
    hi2[2] = np.nan
    refused(basis, np.zeros(n, np.int32), hi2=hi2)
    bad = up.copy()
    bad[int(np.flatnonzero(np.isinf(hi))[0])] = 1
    refused(basis, bad)
    bad = up.copy()
    bad[0] = 2
    refused(basis, bad)
    for index in (-1, n):
        bad = basis.copy()
        bad[3] = index
        refused(bad, up)
    refused(basis, up, eps=-1.0)
    refused(basis, up, eps=np.nan)
    lib = ctx.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    Af = capi.colmajor(A)
    z, zi = np.zeros(n), np.zeros(n, np.int32)
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(dp)   # noqa: E731
    i = lambda a: a.ctypes.data_as(ip)   # noqa: E731
    bi, ui = np.ascontiguousarray(basis, np.int32), np.ascontiguousarray(up, np.int32)
    fn = lib.lp_simplex_bounded_resolve_large
    assert fn(ctx.h, d(Af), m, n, d(b), d(c), d(lo), d(hi), None, i(ui), 1, n, 1e-9, 100, d(z), i(zi), i(zi), d(z),
              i(zi)) == BAD_ARG
    assert fn(ctx.h, d(Af), m, n, d(b), d(c), d(lo), d(hi), i(bi), i(ui), 1, n, 1e-9, 100, None, i(zi), i(zi), d(z),
              i(zi)) == BAD_ARG
    assert fn(None, d(Af), m, n, d(b), d(c), d(lo), d(hi), i(bi), i(ui), 1, n, 1e-9, 100, d(z), i(zi), i(zi), d(z),
              i(zi)) == BAD_ARG
    # the context still works after the refusals, and the LDS entry still refuses the shape
    start = Q.warm(m, n, 1, True, "bound", cold)
    _same(ctx.bounded_resolve_large(*start, True, n - m), Q.ref(("beyond", m, n, 1, True, "bound"), start, True, n - m))
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_resolve(*start, True, n - m)
    assert e.value.code == BAD_ARG
