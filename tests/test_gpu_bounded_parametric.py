"""The parametric right-hand-side and cost paths of bounded-variable LPs on the GPU (lp_basis_bounded_parametric,
lp_basis_bounded_parametric_cost and their batched forms): every output equals tests/ref/bounded_parametric_ref.c's bit
for bit (NaN where it has NaN, signed zeros included) on the named cases as single LPs, on batches of 96 boxed LPs at
shapes that reach both block sizes, in both senses and under three (t_max, max_breaks) settings, chained after
lp_simplex_bounded_batched with run statuses, and with lo = 0, hi = inf against lp_basis_parametric /
lp_basis_parametric_cost; the fits predicates' far side and the refusals on a live context."""
import functools

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_parametric_ref as R
from tests import bounded_ref as B

pytestmark = pytest.mark.gpu

BATCH = 96
# (8, 20) and (64, 192): the smallest and largest of the class; (31, 127) and (32, 127): the last shape of the 256-thread
# kernel and the first of the 1024-thread one ((m+1)(n+1) = 4096, 4224); (13, 41): odd sizes, an even pitch made odd
SHAPES = [(8, 20), (13, 41), (31, 127), (32, 127), (64, 192)]
SETTINGS = ((np.inf, 64), (0.3, 64), (np.inf, 3))


def _call(ctx, path, batched=False):
    return {("rhs", False): ctx.bounded_parametric, ("rhs", True): ctx.bounded_parametric_batched,
            ("cost", False): ctx.bounded_parametric_cost, ("cost", True): ctx.bounded_parametric_cost_batched}[path, batched]


@functools.lru_cache(maxsize=None)
def batch_of(path, m, n, maximize):
    """96 boxed cases of one shape and sense at the reference's optima, stacked; computed once and left unchanged."""
    at = R.stack(R.random_cases(path, m, n, BATCH, first_seed=1 + 1000 * m, maximize=maximize))
    for v in at:
        v.setflags(write=False)
    return at


@pytest.mark.parametrize("t_max", [np.inf, 0.75])
def test_named_cases_as_single_lps(ctx, t_max):
    for name, (path, args, kw, status) in sorted(R.named_cases().items()):
        at, mx = args[:8], args[8]
        kw = dict(dict(t_max=t_max), **kw)
        want = R.parametric(path, *at, maximize=mx, **kw)
        assert status is None or kw["t_max"] != np.inf or want["status"] == status, name
        if want["status"] == R.BAD_ARG:   # a start that is not optimal: the single call raises, the batch reports it
            with pytest.raises(capi.LPError) as e:
                _call(ctx, path)(*at, maximize=mx, **kw)
            assert e.value.code == R.BAD_ARG, name
        else:
            R.same_bits(_call(ctx, path)(*at, maximize=mx, **kw), R.trim(want))
        got = _call(ctx, path, True)(*(v[None] for v in at), maximize=mx, **kw)
        R.same_bits({k: v[0] for k, v in got.items()}, want)


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("maximize", [True, False])
@pytest.mark.parametrize("path", R.PATHS)
def test_batches_of_boxed_lps(ctx, path, maximize, m, n):
    fits = ctx.bounded_parametric_fits if path == "rhs" else ctx.bounded_parametric_cost_fits
    assert fits(m, n)
    at = batch_of(path, m, n, maximize)
    seen = set()
    for t_max, max_breaks in SETTINGS:
        want = R.parametric_batched(path, *at, t_max=t_max, maximize=maximize, max_breaks=max_breaks)
        got = _call(ctx, path, True)(*at, t_max=t_max, maximize=maximize, max_breaks=max_breaks)
        R.same_bits(got, want)
        seen |= set(want["status"].tolist())
        assert (want["nseg"] >= 1).all()
    assert R.OPTIMAL in seen and R.ITER_LIMIT in seen and (R.INFEASIBLE if path == "rhs" else R.UNBOUNDED) in seen
    full = R.parametric_batched(path, *at, maximize=maximize)
    pivots = (full["enter"] >= 0) & (full["leave"] >= 0)
    assert (full["side"][pivots] == 1).any()
    if path == "cost":
        assert (pivots & (full["enter"] == full["leave"])).any()
    one = _call(ctx, path)(*(v[5] for v in at), maximize=maximize)
    R.same_bits(one, R.trim({k: v[5] for k, v in full.items()}))


@pytest.mark.parametrize("path", R.PATHS)
def test_chained_after_the_bounded_solve(ctx, path):
    """run_status of lp_simplex_bounded_batched: infeasible LPs and one with crossed bounds keep their status and get
    nseg 0; the others are walked from the GPU's own bases and flags."""
    m, n, mx = 12, 30, True
    kinds = ["mixed", "infeasible", "mixed", "crossed", "mixed", "infeasible", "mixed", "mixed"]
    lps = [B.boxed_lp(20 + q, m, n, mx, kind) for q, kind in enumerate(kinds)]
    A, b, c, lo, hi = (np.stack([lp[i] for lp in lps]) for i in range(5))
    rng = np.random.default_rng(5)
    direction = rng.uniform(-1.0, 1.0, (len(lps), m if path == "rhs" else n))
    cold = ctx.bounded_batched(A, b, c, lo, hi, mx)
    run = cold["status"]
    assert [int(s) for s, k in zip(run, kinds) if k != "mixed"] == [R.INFEASIBLE] * 3
    assert (run == R.OPTIMAL).sum() >= 3
    # an LP that did not run to an optimum returns a basis of artificials: the call needs indices in [0, n)
    basis = np.where((run == R.OPTIMAL)[:, None], cold["basis"], 0).astype(np.int32)
    at = (A, b, c, lo, hi, basis, cold["at_upper"], direction)
    want = R.parametric_batched(path, *at, maximize=mx, run_status=run)
    got = _call(ctx, path, True)(*at, maximize=mx, run_status=run)
    R.same_bits(got, want)
    assert (got["nseg"][run == R.OPTIMAL] >= 1).all()
    assert (got["nseg"][run != R.OPTIMAL] == 0).all() and np.array_equal(got["status"][run != R.OPTIMAL],
                                                                         run[run != R.OPTIMAL])
    # without the statuses the crossed LP is INFEASIBLE with nseg 0 by the call's own check
    at3 = tuple(v[3:4] for v in at)
    got3 = _call(ctx, path, True)(*at3, maximize=mx)
    R.same_bits(got3, R.parametric_batched(path, *at3, maximize=mx))
    assert got3["status"][0] == R.INFEASIBLE and got3["nseg"][0] == 0


@pytest.mark.parametrize("path", R.PATHS)
def test_without_bounds_it_is_the_plain_parametric(ctx, path):
    plain = ctx.basis_parametric if path == "rhs" else ctx.basis_parametric_cost
    checked = 0
    for p, name, case, boxed in R.plain_named_cases():
        if p != path:
            continue
        A, b, c, basis, direction, mx = case
        for t_max, max_breaks in SETTINGS:
            want = plain(A, b, c, basis, direction, t_max, mx, max_breaks=max_breaks)
            got = _call(ctx, path)(*boxed[:8], t_max=t_max, maximize=mx, max_breaks=max_breaks)
            R.same_bits(got, want)
            assert (got["side"][got["leave"] >= 0] == 0).all() and (got["side"][got["leave"] < 0] == -1).all(), name
            assert not got["at_upper"].any(), name
            checked += 1
    assert checked >= 12


def test_past_the_fits_predicates_nothing_is_launched(ctx):
    for path, fits, (m, n) in (("rhs", ctx.bounded_parametric_fits, (64, 260)),
                               ("cost", ctx.bounded_parametric_cost_fits, (64, 260))):
        while fits(m, n):
            n += 1
        assert fits(m, n - 1) and not fits(m, n)
        A = np.hstack([np.ones((m, n - m)), np.eye(m)])
        b, c, lo, hi = np.ones(m), np.zeros(n), np.zeros(n), np.full(n, np.inf)
        basis, up = np.arange(n - m, n, dtype=np.int32), np.zeros(n, np.int32)
        direction = np.zeros(m if path == "rhs" else n)
        for batched in (False, True):
            at = (A, b, c, lo, hi, basis, up, direction)
            with pytest.raises(capi.LPError) as e:
                _call(ctx, path, batched)(*((v[None] for v in at) if batched else at))
            assert e.value.code == R.BAD_ARG and "fits" in str(e.value), (path, batched)
        # just inside, the same LP runs: the slack basis of max 0.x is optimal, nothing blocks
        at = (A[:, 1:], b, c[1:], lo[1:], hi[1:], basis - 1, up[1:], direction if path == "rhs" else direction[1:])
        got = _call(ctx, path)(*at)
        R.same_bits(got, R.trim(R.parametric(path, *at)))
        assert got["status"] == R.OPTIMAL and len(got["slope"]) == 1


def test_refusals_on_a_live_context_then_a_good_call(ctx):
    name, (path, args, kw, _) = "rhs_upper_blocked", R.named_cases()["rhs_upper_blocked"]
    A, b, c, lo, hi, basis, up, d, mx = args
    n = A.shape[1]
    free = int(np.flatnonzero(np.isinf(hi))[0])
    g = np.zeros(n)

    def changed(v, at, val):
        v = v.copy()
        v[at] = val
        return v

    refusals = [dict(basis=changed(basis, 1, n)), dict(basis=changed(basis, 1, -1)),
                dict(up=changed(np.zeros(n, np.int32), free, 1)), dict(up=changed(up, 0, 2)),
                dict(hi=changed(hi, 0, np.nan)), dict(lo=changed(lo, 0, -np.inf)), dict(lo=changed(lo, 0, np.nan)),
                dict(eps=-1.0), dict(eps=float("nan")), dict(t_max=-1.0), dict(t_max=float("nan")),
                dict(max_breaks=-1)]
    for kw in refusals:
        a = dict(lo=lo, hi=hi, basis=basis, up=up, eps=1e-9, t_max=np.inf, max_breaks=8)
        a.update(kw)
        opts = dict(t_max=a["t_max"], maximize=mx, eps=a["eps"], max_breaks=a["max_breaks"])
        for p, direction in (("rhs", d), ("cost", g)):
            at = (A, b, c, a["lo"], a["hi"], a["basis"], a["up"], direction)
            two = [np.stack([v, v]) for v in (A, b, c, lo, hi, basis, up, direction)]
            for i, v in enumerate(at):
                two[i][1] = v   # only the second LP is bad
            for call in (lambda: _call(ctx, p)(*at, **opts), lambda: _call(ctx, p, True)(*two, **opts),
                         lambda: _call(ctx, p, True)(*two, run_status=np.array([0, 4], np.int32), **opts)):
                with pytest.raises(capi.LPError) as e:
                    call()
                assert e.value.code == R.BAD_ARG, (p, kw)
    # NULL pointers through the C ABI
    lib, h = ctx.lib, ctx.h
    Af = np.ascontiguousarray(A.T).reshape(-1)
    m = A.shape[0]
    i32, f64 = (lambda k: np.zeros(k, np.int32)), (lambda k: np.zeros(k))
    good = [h, capi._d(Af), m, n, capi._d(b), capi._d(c), capi._d(lo), capi._d(hi), capi._i(basis.astype(np.int32)),
            capi._i(up.astype(np.int32)), 1, capi._d(d), np.inf, 1e-9, 8, capi._i(i32(1)), capi._d(f64(10)),
            capi._d(f64(10)), capi._d(f64(9)), capi._i(i32(9)), capi._i(i32(9)), capi._i(i32(9)), capi._i(i32(m)),
            capi._i(i32(n))]
    for pos in (1, 4, 5, 6, 7, 8, 9, 11, 15, 16, 17, 18, 19, 20, 21, 22, 23):
        bad = list(good)
        bad[pos] = None
        assert lib.lp_basis_bounded_parametric(*bad) == R.BAD_ARG, pos
        assert lib.lp_basis_bounded_parametric_cost(*bad) == R.BAD_ARG, pos
    assert lib.lp_basis_bounded_parametric(None, *good[1:]) == R.BAD_ARG
    at = (A, b, c, lo, hi, basis, up, d)
    R.same_bits(ctx.bounded_parametric(*at, maximize=mx), R.trim(R.parametric("rhs", *at, maximize=mx)))
