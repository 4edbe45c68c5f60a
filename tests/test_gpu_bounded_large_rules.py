"""lp_simplex_bounded_large_ex and lp_simplex_bounded_resolve_large_ex on the GPU: the bounded-variable simplex and its
re-solve on the tableau in HBM under Bland's rule and Devex pricing.  Status, x, obj, basis, at_upper and every counter
equal tests/ref/bounded_rules_ref.c's and bounded_resolve_rules_ref.c's bit for bit: beyond the LDS fit on every
outcome, on the cycling LPs, on drive-outs with and without flips, on more rows than the selectors have threads and
(on another LP) more columns than one pricing step, at eps = 0 and under iteration limits that fall among flips and pivots; at shapes
that fit LDS the result is lp_simplex_bounded_ex's / lp_simplex_bounded_resolve_ex's too; Dantzig's rule through _ex
is the entry without a rule; and the refusals.  tests/test_bounded_large_rules_cpu.py shows on the reference that
every input reaches what is claimed here."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_large_cases as K
from tests import bounded_large_rules_cases as X
from tests import bounded_resolve_large_cases as Q
from tests import bounded_rules_ref as RR
from tests.test_gpu_bounded import _same

pytestmark = pytest.mark.gpu

DANTZIG, BLAND, DEVEX = RR.RULES
OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
NAME = X.RULE_NAMES
rules = pytest.mark.parametrize("rule", X.NEW_RULES, ids=[NAME[r] for r in X.NEW_RULES])


def _resolve(ctx, start, maximize, n_orig=None, entry="bounded_resolve_large", **kw):
    """The re-solve, with a refusal (the binding raises) in the form of the reference's BAD_ARG result."""
    try:
        return getattr(ctx, entry)(*start, maximize, n_orig, **kw)
    except capi.LPError as e:
        m, n = start[0].shape
        k = n if n_orig is None else n_orig
        return dict(status=e.code, x=np.full(k, np.nan), basis=np.asarray(start[5]), at_upper=np.asarray(start[6]),
                    obj=np.nan, iters=[0, 0, 0])


@pytest.mark.parametrize("key,rule", X.BOXED_CASES, ids=lambda v: NAME[v] if isinstance(v, int) else "-".join(map(str, v)))
def test_beyond_the_lds_fit(ctx, key, rule):
    m, n = key[:2]
    A, b, c, lo, hi, mx = K.boxed(*key)
    r = X.boxed_ref(key, rule)
    assert (r["status"], r["iters"]) == X.BOXED[key][rule]
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=X.BOXED_MAX_ITER, pivot_rule=NAME[rule]), r)


@rules
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("maximize", [True, False])
def test_both_senses(ctx, rule, seed, maximize):
    A, b, c, lo, hi, _ = K.boxed(160, 320, "mixed", seed, maximize)
    r = X.ref(("sense", seed, maximize), rule, A, b, c, lo, hi, maximize, 160, max_iter=20000)
    _same(ctx.bounded_large(A, b, c, lo, hi, maximize, 160, max_iter=20000, pivot_rule=rule), r)


@rules
def test_more_rows_than_selector_threads(ctx, rule):
    m, n = X.TALL_SHAPE
    A, b, c, lo, hi, mx = K.boxed(m, n, "mixed", 1)
    r = X.tall_ref(rule)
    assert (r["status"], r["iters"]) == X.TALL[rule]
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=X.TALL_MAX_ITER, pivot_rule=rule), r)


@rules
def test_more_columns_than_a_pricing_step(ctx, rule):
    m, n = X.WIDE_KEY[:2]
    A, b, c, lo, hi, mx = K.boxed(*X.WIDE_KEY)
    r = X.wide_ref(rule)
    assert (r["status"], r["iters"]) == X.WIDE[rule]
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=10000, pivot_rule=rule), r)


def test_cycling_lps(ctx):
    A, b, c, lo, hi = RR.cycling_boxed()
    for rule in RR.RULES:
        r = X.cycling_ref(rule)
        assert r["status"] == X.CYCLING[rule][0]
        _same(ctx.bounded_large(A, b, c, lo, hi, True, max_iter=X.CYCLING_MAX_ITER, pivot_rule=rule), r)
    # without a rule the large entry does not finish it
    assert ctx.bounded_large(A, b, c, lo, hi, True, max_iter=X.CYCLING_MAX_ITER)["status"] == ITER_LIMIT
    A, b, c, lo, hi = RR.beale_boxed()
    for rule in (DANTZIG, BLAND):
        r = X.beale_ref(rule)
        assert r["status"] == X.BEALE[rule][0]
        _same(ctx.bounded_large(A, b, c, lo, hi, True, max_iter=X.BEALE_MAX_ITER, pivot_rule=rule), r)


@rules
@pytest.mark.parametrize("key", sorted(X.DRIVEOUT_FLIP))
def test_driveout_after_a_flip(ctx, rule, key):
    A, b, c, lo, hi, mx = K.driveout_with_flip(*key)
    r = X.driveout_flip_ref(key, rule)
    assert r["iters"] == X.DRIVEOUT_FLIP[key][rule]
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=10000, pivot_rule=rule), r)


@rules
@pytest.mark.parametrize("seed", X.DRIVEOUT_SEEDS)
def test_driveout(ctx, rule, seed):
    A, b, c, lo, hi, mx = K.driveout(seed)
    r = X.driveout_ref(seed, rule)
    limit = X.DRIVEOUT_DEVEX_MAX_ITER if rule == DEVEX else 10000
    assert r["status"] == (ITER_LIMIT if rule == DEVEX else OPTIMAL)
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=limit, pivot_rule=rule), r)


def test_dantzig_rule_is_the_entry_without_a_rule(ctx):
    for m, n, kind, seed in K.BEYOND_CASES:
        A, b, c, lo, hi, mx = K.boxed(m, n, kind, seed)
        _same(ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=10000, pivot_rule="dantzig"),
              ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=10000))
    for name in ("cost_max", "bound_max"):   # the primal and the dual branch
        start, mx = X.resolve_start(name)
        g = ctx.bounded_resolve_large(*start, mx, max_iter=10000, pivot_rule="dantzig")
        _same(g, ctx.bounded_resolve_large(*start, mx, max_iter=10000))
        _same(g, X.resolve_ref(name, DANTZIG, start, mx))


@rules
@pytest.mark.parametrize("m,n", Q.LDS_SHAPES)
def test_shapes_that_also_fit_lds(ctx, rule, m, n):
    ran = 0
    for seed in Q.LDS_SEEDS:
        for maximize in (True, False):
            A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, maximize)
            r = X.ref(("lds", m, n, seed, maximize), rule, A, b, c, lo, hi, maximize, n - m)
            g = ctx.bounded_large(A, b, c, lo, hi, maximize, n - m, max_iter=10000, pivot_rule=rule)
            _same(g, r)
            if ctx.bounded_rule_fits(m, n, rule):
                _same(g, ctx.bounded(A, b, c, lo, hi, maximize, n - m, max_iter=10000, pivot_rule=rule))
                ran += 1
            for kind, start in X.lds_warm_starts(m, n, seed, maximize):
                r = X.resolve_ref(("lds", m, n, seed, maximize, kind), rule, start, maximize, n - m)
                g = _resolve(ctx, start, maximize, n - m, max_iter=10000, pivot_rule=rule)
                _same(g, r)
                if r["status"] != BAD_ARG and ctx.bounded_rule_fits(m, n, rule):
                    _same(g, _resolve(ctx, start, maximize, n - m, "bounded_resolve", max_iter=10000, pivot_rule=rule))
    assert ran >= 3


@rules
@pytest.mark.parametrize("name", sorted(X.RESOLVE))
def test_resolve_beyond_the_lds_fit(ctx, rule, name):
    start, mx = X.resolve_start(name)
    r = X.resolve_ref(name, rule, start, mx)
    assert r["iters"] == X.RESOLVE[name][rule]
    _same(ctx.bounded_resolve_large(*start, mx, max_iter=10000, pivot_rule=rule), r)


@rules
def test_identity_anchor(ctx, rule):
    A, b, c, mx, n_orig = K.identity_anchor("gen")
    n = A.shape[1]
    lo, hi = np.zeros(n), np.full(n, np.inf)
    r = X.ref("anchor", rule, A, b, c, lo, hi, mx, n_orig, max_iter=20000)
    assert r["status"] == OPTIMAL and r["iters"][3] == 0
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, n_orig, max_iter=20000, pivot_rule=rule), r)


@rules
def test_eps_zero(ctx, rule):
    A, b, c, lo, hi, mx = K.boxed(160, 320, "mixed", 1)
    r = X.ref("eps0", rule, A, b, c, lo, hi, mx, 160, eps=0.0, max_iter=20000)
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, 160, eps=0.0, max_iter=20000, pivot_rule=rule), r)


@rules
def test_iteration_limits(ctx, rule):
    A, b, c, lo, hi, mx = K.boxed(160, 320, "mixed", 1)
    for k in X.LIMIT_SWEEP:
        r = X.ref(("limit", k), rule, A, b, c, lo, hi, mx, 160, max_iter=k)
        assert r["status"] == ITER_LIMIT
        _same(ctx.bounded_large(A, b, c, lo, hi, mx, 160, max_iter=k, pivot_rule=rule), r)


def test_refusals(ctx):
    A, b, c, lo, hi, mx = (a.copy() if isinstance(a, np.ndarray) else a for a in K.boxed(6, 16, "mixed", 1))
    lib = ctx.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    d = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    i = lambda a: a.ctypes.data_as(ip)   # noqa: E731
    Af = capi.colmajor(A)
    cold = ctx.bounded_large(A, b, c, lo, hi, mx)
    assert cold["status"] == OPTIMAL
    basis, up = np.ascontiguousarray(cold["basis"], np.int32), np.ascontiguousarray(cold["at_upper"], np.int32)
    for rule in (3, -1):   # an unknown rule: LP_BAD_ARG, and no output is written
        x, obj = np.full(16, 7.0), np.full(1, 7.0)
        bo, uo, it = np.full(6, 7, np.int32), np.full(16, 7, np.int32), np.full(4, 7, np.int32)
        assert lib.lp_simplex_bounded_large_ex(ctx.h, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), int(mx), 16, 1e-9, 100,
                                               d(x), i(bo), i(uo), d(obj), i(it), rule) == BAD_ARG
        assert lib.lp_simplex_bounded_resolve_large_ex(ctx.h, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), i(basis), i(up),
                                                       int(mx), 16, 1e-9, 100, d(x), i(bo), i(uo), d(obj), i(it),
                                                       rule) == BAD_ARG
        assert np.all(x == 7.0) and obj[0] == 7.0 and np.all(bo == 7) and np.all(uo == 7) and np.all(it == 7)
        with pytest.raises(capi.LPError) as e:
            ctx.bounded_large(A, b, c, lo, hi, mx, pivot_rule=rule)
        assert e.value.code == BAD_ARG
    # what the plain entry refuses is refused under a rule
    for rule in X.NEW_RULES:
        for bad_lo, bad_hi in ((-np.inf, None), (np.nan, None), (np.inf, None), (None, np.nan)):
            lo2, hi2 = lo.copy(), hi.copy()
            if bad_lo is not None:
                lo2[2] = bad_lo
            if bad_hi is not None:
                hi2[2] = bad_hi
            assert RR.bounded(A, b, c, lo2, hi2, mx, rule=rule)["status"] == BAD_ARG
            with pytest.raises(capi.LPError) as e:
                ctx.bounded_large(A, b, c, lo2, hi2, mx, pivot_rule=rule)
            assert e.value.code == BAD_ARG
            with pytest.raises(capi.LPError) as e:
                ctx.bounded_resolve_large(A, b, c, lo2, hi2, basis, up, mx, pivot_rule=rule)
            assert e.value.code == BAD_ARG
        for kw in (dict(n_orig=17), dict(eps=-1e-9)):
            with pytest.raises(capi.LPError) as e:
                ctx.bounded_large(A, b, c, lo, hi, mx, pivot_rule=rule, **kw)
            assert e.value.code == BAD_ARG
        z, zi = np.zeros(64), np.zeros(64, np.int32)
        assert lib.lp_simplex_bounded_large_ex(ctx.h, d(Af), 6, 16, d(b), d(c), None, d(hi), int(mx), 16, 1e-9, 100,
                                               d(z), i(zi), i(zi), d(z), i(zi), rule) == BAD_ARG
        assert lib.lp_simplex_bounded_large_ex(ctx.h, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), int(mx), 16, 1e-9, 100,
                                               None, i(zi), i(zi), d(z), i(zi), rule) == BAD_ARG
        bad = basis.copy()
        bad[0] = 16
        with pytest.raises(capi.LPError) as e:
            ctx.bounded_resolve_large(A, b, c, lo, hi, bad, up, mx, pivot_rule=rule)
        assert e.value.code == BAD_ARG
        hi2 = hi.copy()
        hi2[3] = lo[3] - 1.0   # crossed bounds: LP_INFEASIBLE without an iteration, as the plain entry
        _same(ctx.bounded_large(A, b, c, lo, hi2, mx, pivot_rule=rule), RR.bounded(A, b, c, lo, hi2, mx, rule=rule))
        # the context still works after the refusals
        _same(ctx.bounded_large(A, b, c, lo, hi, mx, pivot_rule=rule), RR.bounded(A, b, c, lo, hi, mx, rule=rule))
