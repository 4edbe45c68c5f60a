"""lp_simplex_bounded_large on the GPU: the bounded-variable simplex on the tableau in HBM.  Status, x, obj, basis,
at_upper and the four counters equal tests/ref/bounded_ref.c's bit for bit: at shapes that also fit LDS (where the
result is lp_simplex_bounded's too), beyond that fit (an odd tableau width, every outcome, more rows than the selector
has threads, the pure flip path), on dependent rows, on drive-outs with and without flips, under iteration limits that
fall among mixed flips and pivots, at eps = 0; with lo = 0 and hi = inf the result is lp_simplex_two_phase's; and the
refusals.  tests/test_bounded_large_cpu.py shows on the reference that every input reaches what is claimed here."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_large_cases as K
from tests import bounded_ref as R

pytestmark = pytest.mark.gpu

BAD_ARG = R.BAD_ARG


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


@pytest.mark.parametrize("m,n", [(6, 16), (32, 96), (64, 192)])
@pytest.mark.parametrize("maximize", [True, False])
def test_shapes_that_also_fit_lds(ctx, m, n, maximize):
    for seed in (1, 2, 3):
        A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, maximize)
        r = K.ref(("lds", m, n, seed, maximize), A, b, c, lo, hi, maximize, n - m)
        g = ctx.bounded_large(A, b, c, lo, hi, maximize, n - m)
        _same(g, r)
        _same(g, ctx.bounded(A, b, c, lo, hi, maximize, n - m))


@pytest.mark.parametrize("m,n,kind,seed", K.BEYOND_CASES)
def test_beyond_the_lds_fit(ctx, m, n, kind, seed):
    # (67 x 201 still fits LDS: it is in this list for its odd tableau width, which pads a column and splits a pair)
    assert ctx.bounded_fits(m, n) == ((m, n) == (67, 201))
    A, b, c, lo, hi, mx = K.boxed(m, n, kind, seed)
    r = K.ref(("beyond", m, n, kind, seed), A, b, c, lo, hi, mx, n - m)
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, n - m), r)
    if (m, n, kind, seed) in K.BEYOND:
        assert r["status"] == K.BEYOND[(m, n, kind, seed)][0]


@pytest.mark.parametrize("kind,seed", sorted(K.TALL))
def test_more_rows_than_selector_threads(ctx, kind, seed):
    m, n = K.TALL_SHAPE
    A, b, c, lo, hi, mx = K.boxed(m, n, kind, seed)
    r = K.ref(("tall", kind, seed), A, b, c, lo, hi, mx, n - m, max_iter=K.TALL_MAX_ITER)
    assert r["status"] == R.ITER_LIMIT and r["iters"] == K.TALL[(kind, seed)]
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=K.TALL_MAX_ITER), r)


@pytest.mark.parametrize("seed", sorted(K.SINGULAR_FLIPS))
def test_dependent_rows_are_singular(ctx, seed):
    A, b, c, lo, hi, mx = K.singular(seed)
    r = K.ref(("singular", seed), A, b, c, lo, hi, mx)
    assert r["status"] == R.SINGULAR
    _same(ctx.bounded_large(A, b, c, lo, hi, mx), r)


@pytest.mark.parametrize("seed", sorted(K.DRIVEOUT_PIVOTS))
def test_driveout_that_succeeds(ctx, seed):
    A, b, c, lo, hi, mx = K.driveout(seed)
    r = K.ref(("driveout", seed), A, b, c, lo, hi, mx)
    assert r["status"] == R.OPTIMAL and r["iters"][1] == K.DRIVEOUT_PIVOTS[seed]
    _same(ctx.bounded_large(A, b, c, lo, hi, mx), r)


@pytest.mark.parametrize("key", sorted(K.DRIVEOUT_FLIP))
def test_driveout_after_a_flip(ctx, key):
    A, b, c, lo, hi, mx = K.driveout_with_flip(*key)
    r = K.ref(("driveout_flip",) + key, A, b, c, lo, hi, mx)
    assert r["iters"][1] > 0 and r["iters"][3] > 0
    _same(ctx.bounded_large(A, b, c, lo, hi, mx), r)


@pytest.mark.parametrize("which", ["gen", "min_lp"])
def test_identity_anchor_equals_two_phase(ctx, which):
    A, b, c, mx, n_orig = K.identity_anchor(which)
    n = A.shape[1]
    lo, hi = np.zeros(n), np.full(n, np.inf)
    g = ctx.bounded_large(A, b, c, lo, hi, mx, n_orig)
    t = ctx.two_phase(A, b, c, maximize=mx, n_orig=n_orig)
    assert int(g["status"]) == int(t["status"]) == R.OPTIMAL
    _bits_equal(g["x"], t["x"])
    _bits_equal(g["obj"], t["obj"])
    assert np.array_equal(g["basis"], t["basis"])
    assert [int(v) for v in g["iters"][:3]] == [int(v) for v in t["iters"]]
    assert g["iters"][3] == 0 and not np.any(g["at_upper"])
    _same(g, R.bounded(A, b, c, lo, hi, mx, n_orig))


@pytest.mark.parametrize("m,n,top", [(6, 16, 12), (67, 201, 6)])
def test_iteration_limits(ctx, m, n, top):
    A, b, c, lo, hi, mx = K.boxed(m, n, "mixed", 1)
    for k in range(1, top + 1):
        r = K.ref(("limit", m, n, k), A, b, c, lo, hi, mx, n - m, max_iter=k)
        _same(ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=k), r)


@pytest.mark.parametrize("eps", [0.0, 1e-12])
def test_eps_edges(ctx, eps):
    A, b, c, lo, hi, mx = K.boxed(67, 201, "mixed", 1)
    r = K.ref(("eps", eps), A, b, c, lo, hi, mx, 134, eps=eps, max_iter=2000)
    _same(ctx.bounded_large(A, b, c, lo, hi, mx, 134, eps=eps, max_iter=2000), r)


def test_refusals(ctx):
    A, b, c, lo, hi, mx = (a.copy() if isinstance(a, np.ndarray) else a for a in K.boxed(6, 16, "mixed", 1))
    for bad_lo, bad_hi in ((-np.inf, None), (np.nan, None), (np.inf, None), (None, np.nan)):
        lo2, hi2 = lo.copy(), hi.copy()
        if bad_lo is not None:
            lo2[2] = bad_lo
        if bad_hi is not None:
            hi2[2] = bad_hi
        assert R.bounded(A, b, c, lo2, hi2, mx)["status"] == BAD_ARG
        with pytest.raises(capi.LPError) as e:
            ctx.bounded_large(A, b, c, lo2, hi2, mx)
        assert e.value.code == BAD_ARG
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_large(A, b, c, lo, hi, mx, n_orig=17)
    assert e.value.code == BAD_ARG
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_large(A, b, c, lo, hi, mx, eps=-1e-9)
    assert e.value.code == BAD_ARG
    lib = ctx.lib
    dp = C.POINTER(C.c_double)
    Af = capi.colmajor(A)
    z = np.zeros(64)
    zi = np.zeros(64, np.int32)
    d = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    ip = zi.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.lp_simplex_bounded_large(ctx.h, d(Af), 6, 16, d(b), d(c), None, d(hi), int(mx), 16, 1e-9, 100, d(z), ip,
                                        ip, d(z), ip) == BAD_ARG
    assert lib.lp_simplex_bounded_large(ctx.h, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), int(mx), 16, 1e-9, 100, None, ip,
                                        ip, d(z), ip) == BAD_ARG
    # the context still works after the refusals
    _same(ctx.bounded_large(A, b, c, lo, hi, mx), R.bounded(A, b, c, lo, hi, mx))
    # and the LDS entry still refuses the shape the new entry takes
    m, n = 160, 320
    with pytest.raises(capi.LPError) as e:
        ctx.bounded(np.eye(m, n), np.ones(m), np.zeros(n), np.zeros(n), np.ones(n))
    assert e.value.code == BAD_ARG
