"""The bounded-variable simplex on the GPU (lp_simplex_bounded, lp_simplex_bounded_batched): status, x, obj, basis,
at_upper and the four counters equal tests/ref/bounded_ref.c's bit for bit on several shapes, both senses and both block
sizes, on a 4096-LP batch of 64 x 192, on a batch that reaches every outcome, on LPs that end with a fixed column and a
basic variable at its upper bound; with lo = 0 and hi = inf the batch equals lp_simplex_two_phase_batched; and the
refusals (an infinite or NaN bound, a shape beyond lp_simplex_bounded_fits, a null pointer)."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_ref as R

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = 0, 1, 2, 3, 4, 5


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a[~nan], b[~nan])


def _same(g, r):
    assert int(g["status"]) == r["status"]
    assert [int(v) for v in g["iters"]] == r["iters"]
    assert np.array_equal(np.asarray(g["basis"]), r["basis"])
    assert np.array_equal(np.asarray(g["at_upper"]), r["at_upper"])
    _bits_equal(g["x"], r["x"])
    _bits_equal(g["obj"], r["obj"])


def _row(out, k):
    return dict(status=out["status"][k], x=out["x"][k], basis=out["basis"][k], at_upper=out["at_upper"][k],
                obj=out["obj"][k], iters=out["iters"][k])


def _stack(cases):
    return [np.stack([cs[i] for cs in cases]) for i in range(5)]


@pytest.mark.parametrize("m,n", [(4, 12), (8, 20), (16, 48), (32, 96), (48, 120)])
@pytest.mark.parametrize("maximize", [True, False])
def test_shapes_both_senses_and_block_sizes(ctx, m, n, maximize):
    # (m+1)(n+1) <= 4096: four waves ((4, 12), (8, 20), (16, 48)); the others sixteen
    for seed in range(4):
        A, b, c, lo, hi, _ = R.boxed_lp(seed, m, n, maximize)
        r = R.bounded(A, b, c, lo, hi, maximize, n - m)
        _same(ctx.bounded(A, b, c, lo, hi, maximize, n - m), r)


def test_single_lp_outcomes(ctx):
    for kind in ("mixed", "box", "infeasible", "unbounded", "crossed"):
        for seed in range(3):
            A, b, c, lo, hi, mx = R.boxed_lp(seed, 6, 16, kind=kind)
            _same(ctx.bounded(A, b, c, lo, hi, mx), R.bounded(A, b, c, lo, hi, mx))


def test_batch_of_4096_64x192(ctx):
    B, m, n = 4096, 64, 192
    cases = [R.boxed_lp(k, m, n, maximize=True, kind="box" if k % 4 == 1 else "mixed")[:5] for k in range(B)]
    A, b, c, lo, hi = _stack(cases)
    out = ctx.bounded_batched(A, b, c, lo, hi, True, n - m)
    flips = 0
    for k in range(B):
        r = R.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n - m)
        _same(_row(out, k), r)
        flips += r["iters"][3]
    assert flips > 0 and (out["status"] == OPTIMAL).sum() > B // 2


def _outcome_batch(m=6, n=16, max_iter=12):
    """One LP per outcome under one max_iter, found by the reference: optimal, hi < lo, infeasible in phase I,
    unbounded, iteration limit."""
    want = [("mixed", OPTIMAL), ("crossed", INFEASIBLE), ("infeasible", INFEASIBLE), ("unbounded", UNBOUNDED),
            ("mixed", ITER_LIMIT)]
    picked = []
    for kind, status in want:
        for seed in range(400):
            A, b, c, lo, hi, _ = R.boxed_lp(seed, m, n, maximize=True, kind=kind)
            r = R.bounded(A, b, c, lo, hi, True, max_iter=max_iter)
            crossed = bool(np.any(hi < lo))
            if r["status"] == status and crossed == (kind == "crossed"):
                picked.append((A, b, c, lo, hi))
                break
        else:
            raise AssertionError(f"no {kind} case reaching status {status}")
    return picked


def test_batch_reaches_every_outcome(ctx):
    max_iter = 12
    cases = _outcome_batch(max_iter=max_iter)
    A, b, c, lo, hi = _stack(cases)
    out = ctx.bounded_batched(A, b, c, lo, hi, True, max_iter=max_iter)
    assert list(out["status"]) == [OPTIMAL, INFEASIBLE, INFEASIBLE, UNBOUNDED, ITER_LIMIT]
    for k in range(len(cases)):
        _same(_row(out, k), R.bounded(A[k], b[k], c[k], lo[k], hi[k], True, max_iter=max_iter))
    assert list(out["iters"][1]) == [0, 0, 0, 0]   # hi < lo: no iteration
    assert not np.any(cases[2][4] < cases[2][3])    # the phase-I infeasible LP has consistent bounds
    assert np.all(np.isnan(out["x"][1:])) and np.all(np.isnan(out["obj"][1:]))


def test_fixed_column_and_basic_at_upper(ctx):
    hits = 0
    for seed in range(200):
        A, b, c, lo, hi, mx = R.degenerate_lp(seed)
        r = R.bounded(A, b, c, lo, hi, mx)
        if r["status"] != OPTIMAL or not R.basic_at_upper(r, hi):
            continue
        hits += 1
        g = ctx.bounded(A, b, c, lo, hi, mx)
        _same(g, r)
        fixed = np.flatnonzero(lo == hi)
        assert np.array_equal(g["x"][fixed], lo[fixed])
    assert hits >= 2


@pytest.mark.parametrize("m,n", [(8, 20), (32, 96)])
@pytest.mark.parametrize("maximize", [True, False])
def test_identity_anchor_equals_two_phase_batched(ctx, m, n, maximize):
    B = 64
    A, b, c = np.empty((B, m, n)), np.empty((B, m)), np.empty((B, n))
    for k in range(B):
        A[k], b[k], c[k], _ = capi.gen_lp(k, m, n)
        if k % 3 == 0:
            b[k][::2] *= -1.0   # rows that change sign in phase I
    if not maximize:
        c = -c
    lo, hi = np.zeros((B, n)), np.full((B, n), np.inf)
    g = ctx.bounded_batched(A, b, c, lo, hi, maximize, n - m)
    t = ctx.two_phase_batched(A, b, c, maximize, n - m)
    assert np.array_equal(g["status"], t["status"])
    assert np.array_equal(g["basis"], t["basis"])
    assert np.array_equal(g["iters"][:, :3], t["iters"])
    assert not g["iters"][:, 3].any() and not g["at_upper"].any()
    ok = t["status"] == OPTIMAL
    assert ok.any()
    _bits_equal(g["x"][ok], t["x"][ok])
    _bits_equal(g["obj"][ok], t["obj"][ok])


def test_refusals(ctx):
    A, b, c, lo, hi, mx = R.boxed_lp(1, 6, 16)
    for bad_lo, bad_hi in ((-np.inf, None), (np.nan, None), (np.inf, None), (None, np.nan)):
        lo2, hi2 = lo.copy(), hi.copy()
        if bad_lo is not None:
            lo2[2] = bad_lo
        if bad_hi is not None:
            hi2[2] = bad_hi
        assert R.bounded(A, b, c, lo2, hi2, mx)["status"] == BAD_ARG
        with pytest.raises(capi.LPError) as e:
            ctx.bounded(A, b, c, lo2, hi2, mx)
        assert e.value.code == BAD_ARG
        with pytest.raises(capi.LPError):
            ctx.bounded_batched(np.stack([A, A]), np.stack([b, b]), np.stack([c, c]), np.stack([lo, lo2]),
                                np.stack([hi, hi2]), mx)
    m, n = 160, 320
    assert not ctx.bounded_fits(m, n)
    with pytest.raises(capi.LPError) as e:
        ctx.bounded(np.eye(m, n), np.ones(m), np.zeros(n), np.zeros(n), np.ones(n))
    assert e.value.code == BAD_ARG
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_batched(A[None], b[None], c[None], lo[None], hi[None], mx, max_iter=10, n_orig=17)
    assert e.value.code == BAD_ARG
    lib = ctx.lib
    dp = C.POINTER(C.c_double)
    Af = capi.colmajor(A)
    z = np.zeros(64)
    zi = np.zeros(64, np.int32)
    d = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    ip = zi.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.lp_simplex_bounded(ctx.h, d(Af), 6, 16, d(b), d(c), None, d(hi), int(mx), 16, 1e-9, 100, d(z), ip, ip,
                                  d(z), ip) == BAD_ARG
    assert lib.lp_simplex_bounded(ctx.h, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), int(mx), 16, 1e-9, 100, None, ip, ip,
                                  d(z), ip) == BAD_ARG
    assert lib.lp_simplex_bounded_batched(ctx.h, 1, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), int(mx), 16, 1e-9, 100,
                                          d(z), ip, ip, d(z), ip, None) == BAD_ARG
    # the context still works after the refusals
    _same(ctx.bounded(A, b, c, lo, hi, mx), R.bounded(A, b, c, lo, hi, mx))
