"""The dual solution and ranging of bounded-variable LPs on the GPU (lp_basis_bounded_duals, lp_basis_bounded_ranging and
their batched forms): every output equals tests/ref/bounded_sens_ref.c's bit for bit (NaN where it has NaN, signed
zeros included) after ctx.bounded on shapes that reach every path of the kernel, on a 256-LP batch with a crossed LP
and a repeated basis index, at eps = 0 and 1e-12 on degenerate LPs; with lo = 0, hi = inf and no flag the results are
ctx.basis_duals' / ctx.basis_ranging's; the refusals (NULL pointers included) leave the context usable; a flag under
hi = -inf is a crossed bound; and the case where the zero-lower-bound numerator decides a sign bit."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_ref as B
from tests import bounded_sens_ref as S
from tests.test_bounded_sens_cpu import A_SZ, B_SZ, BASIS_SZ, C_SZ
from tests.test_ranging_cpu import _lp

pytestmark = pytest.mark.gpu

OPTIMAL, SINGULAR, INFEASIBLE, BAD_ARG = 0, 3, 4, 5


def _row(out, k):
    return {key: v[k] for key, v in out.items()}


def _same(got, want, keys):
    assert int(got["status"]) == int(want["status"])
    S.same_bits(got, want, keys)


# (13, 40): m no multiple of the 8-row tile; (40, 300): a second 256-column chunk; (72, 150): 512 threads
@pytest.mark.parametrize("m,n", [(4, 12), (13, 40), (32, 96), (40, 300), (72, 150)])
@pytest.mark.parametrize("maximize", [True, False])
def test_shapes_both_senses(ctx, m, n, maximize):
    assert ctx.basis_bounded_fits(m, n)
    kept = 0
    for seed in range(6):
        A, b, c, lo, hi, _ = B.boxed_lp(seed, m, n, maximize)
        sol = ctx.bounded(A, b, c, lo, hi, maximize)
        if sol["status"] != OPTIMAL:
            continue
        kept += 1
        at = (A, b, c, lo, hi, sol["basis"], sol["at_upper"])
        g, q = S.duals(*at), S.ranging(*at, maximize)
        assert g["status"] == OPTIMAL and q["status"] == OPTIMAL
        _same(ctx.bounded_duals(*at), g, S.DUALS_KEYS)
        _same(ctx.bounded_ranging(*at, maximize), q, S.RANGING_KEYS)
        one = tuple(v[None] for v in at)   # a batch of one
        _same(_row(ctx.bounded_duals_batched(*one), 0), g, S.DUALS_KEYS)
        _same(_row(ctx.bounded_ranging_batched(*one, maximize), 0), q, S.RANGING_KEYS)
    assert kept >= 4


def test_batch_of_256_with_a_crossed_lp_and_a_repeated_index(ctx):
    Bn, m, n = 256, 32, 96
    cases = [B.boxed_lp(k, m, n, maximize=True, kind="box" if k % 4 == 1 else "mixed")[:5] for k in range(Bn + 24)]
    A, b, c, lo, hi = (np.stack([cs[i] for cs in cases]) for i in range(5))
    cold = ctx.bounded_batched(A, b, c, lo, hi, True)
    keep = np.flatnonzero(cold["status"] == OPTIMAL)[:Bn]
    assert len(keep) == Bn
    A, b, c, lo, hi = A[keep], b[keep], c[keep], lo[keep].copy(), hi[keep].copy()
    basis, up = cold["basis"][keep].copy(), cold["at_upper"][keep]
    assert up.sum() > Bn   # plenty of columns held at their upper bounds
    j = int(np.flatnonzero(np.isfinite(hi[5]) & (up[5] == 0))[0])
    hi[5, j] = lo[5, j] - 0.25          # LP 5: crossed bounds
    basis[9, 3] = basis[9, 0]           # LP 9: a repeated basis index
    at = (A, b, c, lo, hi, basis, up)
    want_d = S.batched(S.duals, *at)
    want_r = S.batched(S.ranging, *at, True)
    assert want_d["status"][5] == INFEASIBLE and want_d["status"][9] == SINGULAR
    assert (np.delete(want_d["status"], [5, 9]) == OPTIMAL).all()
    assert np.array_equal(want_r["status"], want_d["status"])
    got_d = ctx.bounded_duals_batched(*at)
    got_r = ctx.bounded_ranging_batched(*at, True)
    assert np.array_equal(got_d["status"], want_d["status"]) and np.array_equal(got_r["status"], want_r["status"])
    S.same_bits(got_d, want_d, S.DUALS_KEYS)
    S.same_bits(got_r, want_r, S.RANGING_KEYS)
    assert np.isnan(got_d["x"][5]).all() and (got_r["b_side"][9] == -1).all()
    assert (want_r["b_side"] == 1).sum() > 0   # some variable leaves at its upper bound


@pytest.mark.parametrize("eps", [0.0, 1e-12])
def test_eps_on_degenerate_lps(ctx, eps):
    optimal = 0
    for seed in range(8):
        A, b, c, lo, hi, mx = B.degenerate_lp(seed)
        sol = ctx.bounded(A, b, c, lo, hi, mx)
        at = (A, b, c, lo, hi, sol["basis"], sol["at_upper"])
        if sol["status"] != OPTIMAL:
            # seed 4 is infeasible and its final basis still holds an artificial (an index >= n): there is no basis
            # to analyse, and the reference and both entries refuse it
            assert sol["status"] == INFEASIBLE and (sol["basis"] >= A.shape[1]).any()
            assert S.ranging(*at, mx, eps)["status"] == BAD_ARG and S.duals(*at)["status"] == BAD_ARG
            for call in (lambda: ctx.bounded_ranging(*at, mx, eps), lambda: ctx.bounded_duals(*at)):
                with pytest.raises(capi.LPError) as e:
                    call()
                assert e.value.code == BAD_ARG
            continue
        optimal += 1
        _same(ctx.bounded_ranging(*at, mx, eps), S.ranging(*at, mx, eps), S.RANGING_KEYS)
        _same(ctx.bounded_duals(*at), S.duals(*at), S.DUALS_KEYS)
    assert optimal >= 7


@pytest.mark.parametrize("seed", range(0, 20, 2))
def test_without_bounds_it_is_the_unbounded_analysis(ctx, seed):
    A, b, c, basis, mx = _lp(seed)
    n = A.shape[1]
    lo, hi, up = np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32)
    g, g0 = ctx.bounded_duals(A, b, c, lo, hi, basis, up), ctx.basis_duals(A, b, c, basis)
    _same(g, g0, ("y", "d"))
    assert S.bits(g["w"]) == S.bits(g0["w"])
    q, q0 = ctx.bounded_ranging(A, b, c, lo, hi, basis, up, mx), ctx.basis_ranging(A, b, c, basis, mx)
    _same(q, q0, ("b_lo", "b_hi", "b_leave", "c_lo", "c_hi", "c_enter"))
    assert set(np.unique(q["b_side"]).tolist()) <= {-1, 0}


def test_refusals_then_a_good_call(ctx):
    m, n = 8, 20
    A, b, c, lo, hi, mx = B.boxed_lp(2, m, n)
    sol = ctx.bounded(A, b, c, lo, hi, mx)
    assert sol["status"] == OPTIMAL
    basis, up = sol["basis"], sol["at_upper"]
    free = int(np.flatnonzero(np.isinf(hi))[0])

    def changed(v, at, val):
        v = v.copy()
        v[at] = val
        return v

    refusals = [dict(lo=changed(lo, 0, np.nan)), dict(lo=changed(lo, 0, -np.inf)), dict(lo=changed(lo, 0, np.inf)),
                dict(hi=changed(hi, 0, np.nan)),
                dict(up=changed(up, 0, 2)), dict(up=changed(np.zeros(n, np.int32), free, 1)),
                dict(basis=changed(basis, 1, n)), dict(basis=changed(basis, 1, -1))]
    for kw in refusals:
        args = dict(lo=lo, hi=hi, basis=basis, up=up)
        args.update(kw)
        at = (A, b, c, args["lo"], args["hi"], args["basis"], args["up"])
        two = tuple(np.stack([v, v]) for v in at)
        for call in (lambda: ctx.bounded_duals(*at), lambda: ctx.bounded_ranging(*at, mx),
                     lambda: ctx.bounded_duals_batched(*two), lambda: ctx.bounded_ranging_batched(*two, mx)):
            with pytest.raises(capi.LPError) as e:
                call()
            assert e.value.code == BAD_ARG, kw
    at = (A, b, c, lo, hi, basis, up)
    for eps in (-1e-12, float("nan")):
        with pytest.raises(capi.LPError) as e:
            ctx.bounded_ranging(*at, mx, eps)
        assert e.value.code == BAD_ARG
    big = B.boxed_lp(0, 160, 320)   # beyond lp_basis_bounded_fits
    assert not ctx.basis_bounded_fits(160, 320)
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_duals(*big[:5], np.arange(160, 320, dtype=np.int32), np.zeros(320, np.int32))
    assert e.value.code == BAD_ARG
    # in a batch a bad flag in one LP refuses the whole call, and the context is still good afterwards
    two = [np.stack([v, v]) for v in at]
    two[6][1, free] = 1
    with pytest.raises(capi.LPError):
        ctx.bounded_ranging_batched(*two, mx)
    _same(ctx.bounded_duals(*at), S.duals(*at), S.DUALS_KEYS)
    _same(ctx.bounded_ranging(*at, mx), S.ranging(*at, mx), S.RANGING_KEYS)


def test_null_pointers_are_refused(ctx):
    """Every pointer of the four entries is required: None for any one of them is LP_BAD_ARG with a live context."""
    m, n = 8, 20
    A, b, c, lo, hi, mx = B.boxed_lp(2, m, n)
    sol = ctx.bounded(A, b, c, lo, hi, mx)
    basis, up = np.ascontiguousarray(sol["basis"], np.int32), np.ascontiguousarray(sol["at_upper"], np.int32)
    Af = capi.colmajor(A)
    x, y, d, w = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(1)
    rhs, cost = np.zeros(2 * m), np.zeros(2 * n)
    rv, rs, cv = np.zeros(2 * m, np.int32), np.zeros(2 * m, np.int32), np.zeros(2 * n, np.int32)
    st = np.zeros(1, np.int32)
    dp, ip, lib = capi._d, capi._i, ctx.lib
    ins = [dp(Af), m, n, dp(b), dp(c), dp(lo), dp(hi), ip(basis), ip(up)]
    in_ptrs = (0, 3, 4, 5, 6, 7, 8)
    duals_out = [dp(x), dp(y), dp(d), dp(w)]
    ranging_out = [dp(rhs), ip(rv), ip(rs), dp(cost), ip(cv)]
    calls = [
        (lib.lp_basis_bounded_duals, [ctx.h] + ins + duals_out, [1 + k for k in in_ptrs] + [10, 11, 12, 13]),
        (lib.lp_basis_bounded_duals_batched, [ctx.h, 1] + ins + duals_out + [ip(st)],
         [2 + k for k in in_ptrs] + [11, 12, 13, 14, 15]),
        (lib.lp_basis_bounded_ranging, [ctx.h] + ins + [int(mx), 1e-9] + ranging_out,
         [1 + k for k in in_ptrs] + [12, 13, 14, 15, 16]),
        (lib.lp_basis_bounded_ranging_batched, [ctx.h, 1] + ins + [int(mx), 1e-9] + ranging_out + [ip(st)],
         [2 + k for k in in_ptrs] + [13, 14, 15, 16, 17, 18]),
    ]
    for fn, args, pointers in calls:
        assert fn(*args) == OPTIMAL   # the full call is good
        for at in pointers:
            bad = list(args)
            bad[at] = None
            assert fn(*bad) == BAD_ARG, (fn.__name__, at)
    at = (A, b, c, lo, hi, basis, up)
    _same(ctx.bounded_duals(*at), S.duals(*at), S.DUALS_KEYS)   # the context is still good


def test_a_flag_under_minus_infinity_is_a_crossed_bound(ctx):
    A, b, c, lo, hi, mx = B.boxed_lp(2, 8, 20)
    sol = ctx.bounded(A, b, c, lo, hi, mx)
    hi, up = hi.copy(), sol["at_upper"].copy()
    hi[0], up[0] = -np.inf, 1
    at = (A, b, c, lo, hi, sol["basis"], up)
    g, q = S.duals(*at), S.ranging(*at, mx)
    assert g["status"] == INFEASIBLE and q["status"] == INFEASIBLE
    _same(ctx.bounded_duals(*at), g, S.DUALS_KEYS)
    _same(ctx.bounded_ranging(*at, mx), q, S.RANGING_KEYS)
    one = tuple(v[None] for v in at)
    _same(_row(ctx.bounded_ranging_batched(*one, mx), 0), q, S.RANGING_KEYS)


def test_the_zero_lower_bound_branch_decides_a_sign(ctx):
    """tests/test_bounded_sens_cpu.py's case where -xB / beta and (0.0 - xB) / beta give different bits."""
    lo, hi, up = np.zeros(4), np.full(4, np.inf), np.zeros(4, np.int32)
    at = (A_SZ, B_SZ, C_SZ, lo, hi, BASIS_SZ, up)
    q = ctx.bounded_ranging(*at, True)
    _same(q, S.ranging(*at, True), S.RANGING_KEYS)
    assert q["b_hi"][0] == 0.0 and not np.signbit(q["b_hi"][0])
    _same(ctx.bounded_duals(*at), S.duals(*at), S.DUALS_KEYS)
    _same(q, ctx.basis_ranging(A_SZ, B_SZ, C_SZ, BASIS_SZ, True), ("b_lo", "b_hi", "b_leave", "c_lo", "c_hi", "c_enter"))
