"""Branch-and-bound over variable bounds on the HBM tableau (lp_mip_bounded_solve_large): status, found, x, obj, bound and
the five counters equal tests/ref/mip_bounded_ref.c's bit for bit (NaN positions compared, payloads not): at shapes that
also fit LDS (and there lp_mip_bounded_solve's too), beyond the fit, on rebuild-heavy and dive-only searches, with more
rows and more marked columns than a block has threads (against the recorded reference results), with a zero mask against
lp_simplex_bounded_resolve_large, on every outcome, past level 64, at eps = 0 and 1e-12, and on every refusal.
tests/test_mip_bounded_large_cpu.py shows on the reference alone that these inputs reach what is claimed for them."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_resolve_large_cases as W
from tests import mip_bounded_large_cases as Q
from tests import mip_bounded_ref as R
from tests.test_gpu_mip_bounded import _bits_equal, _outcome_cases, _same

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


@pytest.mark.parametrize("m,n,depth,kind", Q.LDS_SHAPES)
@pytest.mark.parametrize("maximize", [True, False])
def test_shapes_that_also_fit_lds(ctx, m, n, depth, kind, maximize):
    assert ctx.mip_bounded_fits(m, n, depth)
    searched = 0
    for seed in range(3):
        for every in (1, 2):
            got = Q.searched(m, n, seed, maximize, kind, every, max_depth=depth, max_nodes=Q.LDS_NODES)
            if got is None:
                continue
            args, r = got
            kw = dict(max_depth=depth, max_nodes=Q.LDS_NODES)
            g = ctx.mip_bounded_solve_large(*args, **kw)
            _same(g, r)
            _same(g, _as_ref(ctx.mip_bounded_solve(*args, **kw)))
            searched += r["stats"][0] > 1
    assert searched > 0


def _as_ref(g):
    return dict(g, stats=tuple(int(v) for v in g["stats"]))


@pytest.mark.parametrize("m,n,seed,maximize,nodes", Q.BEYOND)
def test_beyond_the_lds_fit(ctx, m, n, seed, maximize, nodes):
    kw = dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes)
    args, r = Q.searched(m, n, seed, maximize, "mixed", 2, **kw)
    g = ctx.mip_bounded_solve_large(*args, **kw)
    _same(g, r)
    if (m, n) == (160, 320):
        assert not ctx.mip_bounded_fits(m, n, 0)
        assert (g["status"], g["stats"][0]) == Q.BEYOND_160[(seed, maximize)]
    if ctx.mip_bounded_fits(m, n, Q.BEYOND_DEPTH):
        _same(g, _as_ref(ctx.mip_bounded_solve(*args, **kw)))


def test_first_children_that_end_infeasible(ctx):
    m, n, seed, maximize, every, nodes = Q.BEYOND_INFEASIBLE_DIVES
    kw = dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes)
    args, r = Q.searched(m, n, seed, maximize, "mixed", every, **kw)
    _same(ctx.mip_bounded_solve_large(*args, **kw), r)


@pytest.mark.parametrize("seed", Q.BOX_SEEDS)
@pytest.mark.parametrize("depth", [8, 64])
def test_rebuild_heavy_and_dive_only(ctx, seed, depth):
    kw = dict(max_depth=depth, max_nodes=60)
    args, r = Q.searched(160, 320, seed, True, "box", 1, **kw)
    g = ctx.mip_bounded_solve_large(*args, **kw)
    _same(g, r)
    assert g["stats"][4] == (8 if depth == 8 else 59) and not g["found"] and np.isfinite(g["bound"])


@pytest.mark.parametrize("depth,nodes", sorted(Q.TALL_RUNS))
def test_more_rows_and_marked_columns_than_a_block_has_threads(ctx, depth, nodes):
    m, n = Q.TALL_SHAPE
    assert m > 1024 and Q.TALL_K > 1024
    want = Q.tall_fixture()[(depth, nodes)]
    assert (want["status"], want["stats"]) == Q.TALL_RUNS[(depth, nodes)]
    g = ctx.mip_bounded_solve_large(*Q.tall_args(1), max_depth=depth, max_nodes=nodes, max_iter=Q.TALL_MAX_ITER)
    _same(g, want)


@pytest.mark.parametrize("kind", ["bound", "cost"])
def test_zero_mask_is_the_bounded_resolve(ctx, kind):
    """bound: the start is dual feasible only (the dual loop); cost: primal feasible only (the primal loop and its
    flips).  Q.zero_mask_start says which bounds are rounded."""
    m, n = 160, 320
    A, b, c, lo, hi, basis, up, mask = Q.zero_mask_start(kind)
    g = ctx.bounded_resolve_large(A, b, c, lo, hi, basis, up, True, n - m)
    out = ctx.mip_bounded_solve_large(A, b, c, lo, hi, basis, up, np.zeros(n, np.int32), True, n - m)
    assert out["status"] == g["status"] == OPTIMAL and out["found"] == 1
    assert tuple(out["stats"][1:4]) == tuple(int(v) for v in g["iters"])
    assert out["stats"][0] == 1 and out["stats"][4] == 0
    assert g["iters"][0 if kind == "bound" else 1] > 0 and (kind == "bound" or g["iters"][2] > 0)
    _bits_equal(out["x"], g["x"])
    _bits_equal(out["obj"], g["obj"])
    _bits_equal(out["bound"], g["obj"])
    if kind == "bound":   # with the real mask the same start is searched
        kw = dict(max_depth=64, max_nodes=20)
        r = Q.ref(("zero-mask", kind), A, b, c, lo, hi, basis, up, mask, True, n - m, **kw)
        _same(ctx.mip_bounded_solve_large(A, b, c, lo, hi, basis, up, mask, True, n - m, **kw), r)


def test_every_outcome_one_at_a_time(ctx):
    A, b, c, lo, hi, basis, up, mask, kinds, kw, expect = _outcome_cases()
    assert len(kinds) == 9, kinds
    for k, kind in enumerate(kinds):
        args = (A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, 4)
        r = R.mip(*args, **kw)
        assert r["status"] == expect[kind], kind
        if kind == "no_valid_start":
            with pytest.raises(capi.LPError):
                ctx.mip_bounded_solve_large(*args, **kw)
            continue
        g = ctx.mip_bounded_solve_large(*args, **kw)
        _same(g, r)
        if kind == "depth_limit":
            assert g["bound"] > g["obj"]
        if kind == "integer_infeasible":
            assert g["stats"][0] > 1


def test_singular_start_at_160x320(ctx):
    m, n = 160, 320
    cases = {name: start for name, start, _, _ in W.outcomes_160(W.cold_ref(m, n, 1, True))}
    A, b, c, lo, hi, basis, up = cases["singular"]
    mask = np.zeros(n, np.int32)
    r = Q.ref(("singular-160",), A, b, c, lo, hi, basis, up, mask, True, n - m)
    assert r["status"] == SINGULAR
    _same(ctx.mip_bounded_solve_large(A, b, c, lo, hi, basis, up, mask, True, n - m), r)


def test_search_past_level_64(ctx):
    A, b, c, lo, hi, mask, maximize, root = R.deep_case()
    k = R.DEEP_K
    args = (A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, k)
    r = Q.ref(("deep",), *args, max_depth=1024)
    g = ctx.mip_bounded_solve_large(*args, max_depth=1024)
    _same(g, r)
    _same(g, _as_ref(ctx.mip_bounded_solve(*args, max_depth=1024)))
    assert g["status"] == OPTIMAL and g["stats"][4] > 64


@pytest.mark.parametrize("eps", [0.0, 1e-12])
def test_eps_zero_and_tiny(ctx, eps):
    kw = dict(eps=eps, max_depth=64, max_nodes=30)
    args, r = Q.searched(67, 201, 1, True, "mixed", 2, **kw)
    _same(ctx.mip_bounded_solve_large(*args, **kw), r)


def test_refusals(ctx):
    m, n = 160, 320
    args, r = Q.searched(m, n, 2, True, "mixed", 2, max_depth=64, max_nodes=60)
    A, b, c, lo, hi, basis, up, mask, maximize, no = args
    for bad in (dict(max_depth=1025), dict(max_depth=-1), dict(max_nodes=0), dict(int_tol=0.5), dict(gap=-1.0),
                dict(eps=-1.0), dict(int_tol=float("nan")), dict(gap=float("nan")), dict(eps=float("nan"))):
        with pytest.raises(capi.LPError):
            ctx.mip_bounded_solve_large(*args, **bad)
    j = int(np.flatnonzero(mask)[0])
    frac = hi.copy()
    frac[j] = np.floor(lo[j]) + 2.5
    with pytest.raises(capi.LPError):
        ctx.mip_bounded_solve_large(A, b, c, lo, frac, basis, up, mask, maximize, no)
    beyond = mask.copy()
    beyond[n - 1] = 1
    two = mask.copy()
    two[j] = 2
    flagged = up.copy()
    flagged[int(np.flatnonzero(np.isinf(hi))[0])] = 1
    outside = basis.copy()
    outside[0] = n
    nan_hi, inf_lo = hi.copy(), lo.copy()
    nan_hi[1] = np.nan
    inf_lo[1] = -np.inf
    for a in ((A, b, c, lo, hi, basis, up, beyond, maximize, no), (A, b, c, lo, hi, basis, up, two, maximize, no),
              (A, b, c, lo, hi, basis, flagged, mask, maximize, no), (A, b, c, lo, hi, outside, up, mask, maximize, no),
              (A, b, c, lo, nan_hi, basis, up, mask, maximize, no), (A, b, c, inf_lo, hi, basis, up, mask, maximize, no),
              (A, b, c, lo, hi, basis, up, mask, maximize, 0), (A, b, c, lo, hi, basis, up, mask, maximize, n + 1)):
        with pytest.raises(capi.LPError):
            ctx.mip_bounded_solve_large(*a)
    # crossed bounds at the root are no refusal: LP_INFEASIBLE after one node, nothing found, as the reference
    crossed = hi.copy()
    crossed[j] = lo[j] - 1.0
    rc = Q.ref(("crossed-160",), A, b, c, lo, crossed, basis, up, mask, maximize, no)
    assert rc["status"] == INFEASIBLE and rc["stats"][0] == 1 and not rc["found"]
    _same(ctx.mip_bounded_solve_large(A, b, c, lo, crossed, basis, up, mask, maximize, no), rc)
    # NULL pointers and a NULL context through the raw symbol: LP_BAD_ARG, nothing launched
    fn = ctx.lib.lp_mip_bounded_solve_large
    d = np.zeros(16).ctypes.data_as(C.POINTER(C.c_double))
    i = np.zeros(16, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    good = [ctx.h, d, 2, 4, d, d, d, d, i, i, 1, 4, i, 1e-9, 1e-6, 1e-9, 4, 10, 10, d, d, d, i, i]
    assert fn(None, *good[1:]) == BAD_ARG
    for pos in (1, 4, 5, 6, 7, 8, 9, 12, 19, 20, 21, 22, 23):
        call = list(good)
        call[pos] = None
        assert fn(*call) == BAD_ARG, pos
    # the context still solves, and the LDS entry still refuses the shape
    _same(ctx.mip_bounded_solve_large(*args, max_depth=64, max_nodes=60), r)
    with pytest.raises(capi.LPError):
        ctx.mip_bounded_solve(*args, max_depth=0)
