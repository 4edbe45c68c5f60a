"""The dual solution and ranging of a bounded-variable LP beyond one workgroup's LDS (lp_basis_bounded_duals_large,
lp_basis_bounded_ranging_large): every output equals tests/ref/bounded_sens_ref.c's bit for bit (NaN where it has NaN,
signed zeros included) at the basis and flags ctx.bounded_large returns, and at 67 x 201 the LDS entries' as well; on
integer bases whose RHS and cost ratios tie across the kernels' row subsets, row blocks and column chunks, for both
senses and at eps = 0; with lo = 0, hi = inf and no flag the results are the plain HBM path's (ctx.basis_duals,
ctx.basis_ranging); the statuses and the refusals are the LDS entries', and the context stays usable after each."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_large_cases as Q
from tests import bounded_sens_large_cases as L
from tests import bounded_sens_ref as S

pytestmark = pytest.mark.gpu

OPTIMAL, SINGULAR, INFEASIBLE, BAD_ARG = 0, 3, 4, 5


def _same(got, want, keys):
    assert int(got["status"]) == int(want["status"])
    S.same_bits(got, want, keys)


@pytest.mark.parametrize("m,n,kind,seed", L.SOLVED)
def test_solved_cases(ctx, m, n, kind, seed):
    A, b, c, lo, hi, mx = Q.boxed(m, n, kind, seed)
    sol = ctx.bounded_large(A, b, c, lo, hi, mx)
    assert sol["status"] == OPTIMAL
    at = (A, b, c, lo, hi, sol["basis"], sol["at_upper"])
    g, q = S.duals(*at), S.ranging(*at, mx)
    assert g["status"] == OPTIMAL and q["status"] == OPTIMAL
    gd, gr = ctx.bounded_duals_large(*at), ctx.bounded_ranging_large(*at, mx)
    _same(gd, g, S.DUALS_KEYS)
    _same(gr, q, S.RANGING_KEYS)
    if (m, n) == (67, 201):
        assert ctx.basis_bounded_fits(67, 201)
        _same(gd, ctx.bounded_duals(*at), S.DUALS_KEYS)
        _same(gr, ctx.bounded_ranging(*at, mx), S.RANGING_KEYS)
    else:
        assert not ctx.basis_bounded_fits(m, n)


@pytest.mark.parametrize("seed,m,n", L.TIES)
def test_tie_cases(ctx, seed, m, n):
    at = L.tie(seed, m, n)
    _same(ctx.bounded_duals_large(*at), L.duals(("tie", seed), *at), S.DUALS_KEYS)
    for mx in (False, True):
        for eps in (1e-9, 0.0):
            want = L.ranging(("tie", seed), *at, maximize=mx, eps=eps)
            assert want["status"] == OPTIMAL
            _same(ctx.bounded_ranging_large(*at, mx, eps), want, S.RANGING_KEYS)


def test_without_bounds_it_is_the_plain_hbm_analysis(ctx):
    m, n = 160, 320
    A, b, c, lo, hi, mx = Q.boxed(m, n, "mixed", 1)
    basis = ctx.bounded_large(A, b, c, lo, hi, mx)["basis"]   # any non-singular basis does
    lo, hi, up = np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32)
    g, g0 = ctx.bounded_duals_large(A, b, c, lo, hi, basis, up), ctx.basis_duals(A, b, c, basis)
    _same(g, g0, ("y", "d"))
    assert S.bits(g["w"]) == S.bits(g0["w"])
    for maximize in (False, True):
        q = ctx.bounded_ranging_large(A, b, c, lo, hi, basis, up, maximize)
        _same(q, ctx.basis_ranging(A, b, c, basis, maximize), ("b_lo", "b_hi", "b_leave", "c_lo", "c_hi", "c_enter"))
        assert set(np.unique(q["b_side"]).tolist()) <= {-1, 0}


def _good_call(ctx, at, mx):
    _same(ctx.bounded_duals_large(*at), L.duals("good", *at), S.DUALS_KEYS)
    _same(ctx.bounded_ranging_large(*at, mx), L.ranging("good", *at, maximize=mx), S.RANGING_KEYS)


@pytest.fixture(scope="module")
def solved_160(ctx):
    """(A, b, c, lo, hi, basis, at_upper), maximize of the 160 x 320 "mixed" case 1 at ctx.bounded_large's result."""
    A, b, c, lo, hi, mx = Q.boxed(160, 320, "mixed", 1)
    sol = ctx.bounded_large(A, b, c, lo, hi, mx)
    assert sol["status"] == OPTIMAL
    return (A, b, c, lo, hi, sol["basis"], sol["at_upper"]), mx


def _changed(v, at, val):
    v = np.array(v)
    v[at] = val
    return v


def test_statuses_at_160x320(ctx, solved_160):
    at, mx = solved_160
    A, b, c, lo, hi, basis, up = at
    j = int(np.flatnonzero(np.isfinite(hi) & (up == 0))[0])
    A1, b1, c1, lo1, hi1, _ = Q.singular(1)   # the same bounds; rows 0 and m-1 of A are equal, so is every basis's
    cases = [((A, b, c, lo, _changed(hi, j, lo[j] - 0.25), basis, up), INFEASIBLE),
             ((A, b, c, lo, hi, _changed(basis, 3, basis[0]), up), SINGULAR),
             ((A1, b1, c1, lo1, hi1, basis, up), None)]   # whatever the reference says
    for bad, status in cases:
        g, q = S.duals(*bad), S.ranging(*bad, mx)
        assert g["status"] == q["status"] and (status is None or g["status"] == status)
        gd, gr = ctx.bounded_duals_large(*bad), ctx.bounded_ranging_large(*bad, mx)
        _same(gd, g, S.DUALS_KEYS)
        _same(gr, q, S.RANGING_KEYS)
        if g["status"] != OPTIMAL:
            assert np.isnan(gd["x"]).all() and np.isnan(gd["w"]) and np.isnan(gr["c_lo"]).all()
            assert (gr["b_leave"] == -1).all() and (gr["b_side"] == -1).all() and (gr["c_enter"] == -1).all()
        _good_call(ctx, at, mx)


def test_refusals_at_160x320(ctx, solved_160):
    at, mx = solved_160
    A, b, c, lo, hi, basis, up = at
    n = 320
    free = int(np.flatnonzero(np.isinf(hi))[0])
    refusals = [dict(lo=_changed(lo, 0, np.nan)), dict(lo=_changed(lo, 0, -np.inf)), dict(lo=_changed(lo, 0, np.inf)),
                dict(hi=_changed(hi, 0, np.nan)),
                dict(up=_changed(up, 0, 2)), dict(up=_changed(np.zeros(n, np.int32), free, 1)),
                dict(basis=_changed(basis, 1, n)), dict(basis=_changed(basis, 1, -1))]
    for kw in refusals:
        args = dict(lo=lo, hi=hi, basis=basis, up=up)
        args.update(kw)
        bad = (A, b, c, args["lo"], args["hi"], args["basis"], args["up"])
        assert S.duals(*bad)["status"] == BAD_ARG and S.ranging(*bad, mx)["status"] == BAD_ARG
        for call in (lambda: ctx.bounded_duals_large(*bad), lambda: ctx.bounded_ranging_large(*bad, mx)):
            with pytest.raises(capi.LPError) as e:
                call()
            assert e.value.code == BAD_ARG, kw
    for eps in (-1e-12, float("nan")):
        with pytest.raises(capi.LPError) as e:
            ctx.bounded_ranging_large(*at, mx, eps)
        assert e.value.code == BAD_ARG
    _good_call(ctx, at, mx)


def test_null_pointers_are_refused(ctx, solved_160):
    at, mx = solved_160
    A, b, c, lo, hi, basis, up = at
    m, n = A.shape
    basis, up = np.ascontiguousarray(basis, np.int32), np.ascontiguousarray(up, np.int32)
    Af = capi.colmajor(A)
    x, y, d, w = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(1)
    rhs, cost = np.zeros(2 * m), np.zeros(2 * n)
    rv, rs, cv = np.zeros(2 * m, np.int32), np.zeros(2 * m, np.int32), np.zeros(2 * n, np.int32)
    dp, ip, lib = capi._d, capi._i, ctx.lib
    f = [np.ascontiguousarray(v, np.float64) for v in (b, c, lo, hi)]
    ins = [dp(Af), m, n, dp(f[0]), dp(f[1]), dp(f[2]), dp(f[3]), ip(basis), ip(up)]
    in_ptrs = [1 + k for k in (0, 3, 4, 5, 6, 7, 8)]
    calls = [(lib.lp_basis_bounded_duals_large, [ctx.h] + ins + [dp(x), dp(y), dp(d), dp(w)], in_ptrs + [10, 11, 12, 13]),
             (lib.lp_basis_bounded_ranging_large, [ctx.h] + ins + [int(mx), 1e-9, dp(rhs), ip(rv), ip(rs), dp(cost), ip(cv)],
              in_ptrs + [12, 13, 14, 15, 16])]
    for fn, args, pointers in calls:
        for k in pointers:
            bad = list(args)
            bad[k] = None
            assert fn(*bad) == BAD_ARG, (fn.__name__, k)
        assert fn(*args) == OPTIMAL   # the full call is good, and the context still is
    want = L.duals("good", *at)
    assert np.array_equal(S.bits(x), S.bits(want["x"])) and S.bits(w[0]) == S.bits(want["w"])
