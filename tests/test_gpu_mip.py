"""Depth-first branch-and-bound on the GPU (lp_mip_solve, lp_mip_solve_batched, lp_batched_mip): status, found, x,
obj, bound and the four counters equal tests/ref/mip_ref.c's on several shapes, both senses, both block sizes and
mixed masks, on a 4096-problem batch, on a batch that reaches every outcome, from plain and re-solve batch runs,
with a wide gap, and the refusals (Bland's rule, a shape beyond lp_mip_fits)."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import mip_ref as M

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = 0, 1, 2, 3, 4, 5


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a[~nan], b[~nan])


def _same(g, r):
    assert g["status"] == r["status"]
    assert g["found"] == r["found"]
    assert tuple(int(v) for v in g["stats"]) == r["stats"]
    _bits_equal(g["x"], r["x"])
    _bits_equal(g["obj"], r["obj"])
    _bits_equal(g["bound"], r["bound"])


def _row(out, k):
    return dict(status=int(out["status"][k]), found=int(out["found"][k]), x=out["x"][k], obj=out["obj"][k],
                bound=out["bound"][k], stats=out["stats"][k])


def _gen(seed, m, n, maximize):
    A, b, c, basis = capi.gen_lp(seed, m, n)
    return A, b, (c if maximize else -c), basis


@pytest.mark.parametrize("m,n,depth", [(4, 10, 6), (8, 20, 12), (16, 40, 24), (24, 60, 32)])
@pytest.mark.parametrize("maximize", [True, False])
def test_shapes_both_senses_and_block_sizes(ctx, m, n, depth, maximize):
    # (24, 60, 32): 57 x 93 > 4096, sixteen waves; the others four
    no = n - m
    masks = [np.r_[np.ones(no), np.zeros(m)], np.r_[np.arange(no) % 2, np.zeros(m)]]
    for seed in range(3):
        A, b, c, basis = _gen(seed, m, n, maximize)
        for mask in masks:
            mask = mask.astype(np.int32)
            r = M.mip(A, b, c, basis, mask, maximize, no, max_depth=depth, max_nodes=300)
            g = ctx.mip(A, b, c, basis, mask, maximize, no, max_depth=depth, max_nodes=300)
            _same(g, r)


@pytest.mark.parametrize("s", range(24))
def test_knapsacks_match_the_reference(ctx, s):
    rng = np.random.default_rng(1000 + s)
    m, k = int(rng.integers(2, 7)), int(rng.integers(4, 11))
    A, b, c, basis, mask = M.knapsack(s, m, k, box=2 if k > 7 else 3)
    for maximize, cc in ((True, c), (False, -c)):
        r = M.mip(A, b, cc, basis, mask, maximize, k)
        _same(ctx.mip(A, b, cc, basis, mask, maximize, k), r)
        assert r["status"] == OPTIMAL


def test_batch_of_4096(ctx):
    B, m, n = 4096, 16, 40
    A, b, c, basis = np.empty((B, m, n)), np.empty((B, m)), np.empty((B, n)), np.empty((B, m), np.int32)
    for k in range(B):
        A[k], b[k], c[k], basis[k] = capi.gen_lp(k, m, n)
    mask = np.r_[np.ones(n - m), np.zeros(m)].astype(np.int32)
    out = ctx.mip_batched(A, b, c, basis, mask, True, n - m, max_depth=24, max_nodes=60)
    for k in range(B):
        r = M.mip(A[k], b[k], c[k], basis[k], mask, True, n - m, max_depth=24, max_nodes=60)
        _same(_row(out, k), r)


def _mixed_cases():
    """3 x 7 problems ([A0 | I], 4 integer columns) and the limits max_depth 4, max_nodes 20, max_iter 4 under which
    the reference reaches every outcome; returns (A, b, c, basis, mask, kinds, limits), one problem per outcome."""
    kw = dict(max_depth=4, max_nodes=20, max_iter=4)
    mask = np.r_[np.ones(4), np.zeros(3)].astype(np.int32)
    I3, basis = np.eye(3), np.array([4, 5, 6], np.int32)
    fixed = {
        # 2 x0 + 2 x1 = 1: no integer point, the relaxation feasible
        "integer_infeasible": (np.array([[2.0, 2, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 1, 0], [0, 0, 1, 1, 0, 0, 1]]),
                               np.array([1.0, 5, 3]), np.array([1.0, 1, 1, 1, 0, 0, 0]), np.array([0, 5, 6], np.int32)),
        # b0 < 0 and c <= 0: the slack basis is dual feasible, the root infeasible
        "root_infeasible": (np.hstack([np.ones((3, 4)), I3]), np.array([-1.0, 3, 3]),
                            np.array([-1.0, -2, -1, -3, 0, 0, 0]), basis),
        # column 0 has no positive entry and c_0 > 0
        "unbounded": (np.hstack([-np.ones((3, 1)), np.ones((3, 3)), I3]), np.array([2.0, 3, 4]),
                      np.array([1.0, 1, 1, 1, 0, 0, 0]), basis),
    }
    cases = {k: v for k, v in fixed.items()}
    want = ("optimal", "node_limit", "depth_limit", "iter_limit")
    for s in range(2000):
        if all(k in cases for k in want):
            break
        A, b, c, bs, _ = M.knapsack(7000 + s, 3, 4, box=4)
        r = M.mip(A, b, c, bs, mask, True, 4, **kw)
        st, nodes = r["status"], r["stats"][0]
        if st == OPTIMAL:
            kind = "optimal"
        elif st == ITER_LIMIT and nodes == kw["max_nodes"]:
            kind = "node_limit"
        elif st == ITER_LIMIT and nodes == 1:
            kind = "iter_limit"
        elif st == ITER_LIMIT and r["found"] and r["bound"] > r["obj"] and r["stats"][3] == kw["max_depth"]:
            kind = "depth_limit"
        else:
            continue
        cases.setdefault(kind, (A, b, c, bs))
    kinds = sorted(cases)
    A = np.stack([cases[k][0] for k in kinds])
    b = np.stack([cases[k][1] for k in kinds])
    c = np.stack([cases[k][2] for k in kinds])
    bs = np.stack([cases[k][3] for k in kinds])
    return A, b, c, bs, mask, kinds, kw


def test_mixed_outcome_batch(ctx):
    A, b, c, basis, mask, kinds, kw = _mixed_cases()
    assert len(kinds) == 7, kinds
    out = ctx.mip_batched(A, b, c, basis, mask, True, 4, **kw)
    expect = dict(optimal=OPTIMAL, integer_infeasible=INFEASIBLE, root_infeasible=INFEASIBLE, unbounded=UNBOUNDED,
                  node_limit=ITER_LIMIT, depth_limit=ITER_LIMIT, iter_limit=ITER_LIMIT)
    for k, kind in enumerate(kinds):
        r = M.mip(A[k], b[k], c[k], basis[k], mask, True, 4, **kw)
        assert r["status"] == expect[kind], kind
        _same(_row(out, k), r)
    dl = _row(out, kinds.index("depth_limit"))
    assert dl["bound"] > dl["obj"]


def test_one_shot_batch_of_one_and_handles_agree(ctx):
    B, m, n = 6, 8, 20
    A, b, c, basis = np.empty((B, m, n)), np.empty((B, m)), np.empty((B, n)), np.empty((B, m), np.int32)
    for k in range(B):
        A[k], b[k], c[k], basis[k] = capi.gen_lp(50 + k, m, n)
    mask = np.r_[np.ones(n - m), np.zeros(m)].astype(np.int32)
    kw = dict(max_depth=16, max_nodes=400)
    batch = ctx.mip_batched(A, b, c, basis, mask, True, n - m, **kw)
    for k in range(B):
        one = ctx.mip(A[k], b[k], c[k], basis[k], mask, True, n - m, **kw)
        b1 = ctx.mip_batched(A[k:k + 1], b[k:k + 1], c[k:k + 1], basis[k:k + 1], mask, True, n - m, **kw)
        r = M.mip(A[k], b[k], c[k], basis[k], mask, True, n - m, **kw)
        _same(one, r)
        _same(_row(b1, 0), r)
        _same(_row(batch, k), r)
    # the handles start from the final bases of their runs: the reference from the same bases
    for h in (ctx.batched_problem(A, b, c, basis, True, n - m), ctx.batched_resolve_problem(A, b, c, basis, True, n - m)):
        h.run()
        final = h.download()
        out = h.mip(mask, **kw)
        for k in range(B):
            assert final["status"][k] == OPTIMAL
            r = M.mip(A[k], b[k], c[k], final["basis"][k], mask, True, n - m, **kw)
            _same(_row(out, k), r)
        h.free()


def test_handle_keeps_a_failed_run_status(ctx):
    A, b, c, basis, _, kinds, _ = _mixed_cases()
    k = kinds.index("unbounded")
    mask = np.r_[np.ones(4), np.zeros(3)].astype(np.int32)
    h = ctx.batched_resolve_problem(A[k:k + 1], b[k:k + 1], c[k:k + 1], basis[k:k + 1], True, 4)
    h.run()
    out = h.mip(mask)
    assert out["status"][0] == UNBOUNDED and out["found"][0] == 0 and np.isnan(out["obj"][0])
    assert tuple(out["stats"][0]) == (0, 0, 0, 0)
    h.free()


def test_wide_gap_prunes_more(ctx):
    A, b, c, basis, mask = M.knapsack(11, 4, 8, box=3)
    tight = ctx.mip(A, b, c, basis, mask, True, 8)
    wide = ctx.mip(A, b, c, basis, mask, True, 8, gap=1.0)
    _same(tight, M.mip(A, b, c, basis, mask, True, 8))
    _same(wide, M.mip(A, b, c, basis, mask, True, 8, gap=1.0))
    assert wide["stats"][0] <= tight["stats"][0]
    assert wide["found"] == 1 and wide["obj"] >= tight["obj"] - 1.0


def test_wide_gap_prunes_strictly_fewer_somewhere(ctx):
    fewer = 0
    for s in range(12):
        A, b, c, basis, mask = M.knapsack(200 + s, 4, 8, box=3)
        t = ctx.mip(A, b, c, basis, mask, True, 8)
        w = ctx.mip(A, b, c, basis, mask, True, 8, gap=1.0)
        _same(w, M.mip(A, b, c, basis, mask, True, 8, gap=1.0))
        fewer += w["stats"][0] < t["stats"][0]
    assert fewer > 0


def test_bland_batch_is_refused(ctx):
    A, b, c, basis = capi.gen_lp(1, 4, 10)
    p = ctx.batched_problem(A[None], b[None], c[None], basis[None], True, 6)
    p.set_pivot_rule("bland")
    p.run()
    with pytest.raises(capi.LPError) as e:
        p.mip(np.r_[np.ones(6), np.zeros(4)].astype(np.int32))
    p.free()


def test_shape_beyond_lds_is_refused(ctx):
    m, n = 120, 240
    assert not ctx.mip_fits(m, n, 32)
    A, b, c, basis = capi.gen_lp(0, m, n)
    with pytest.raises(capi.LPError):
        ctx.mip(A, b, c, basis, np.zeros(n, np.int32), True, n - m, max_depth=32)


def test_handle_before_run_is_refused(ctx):
    A, b, c, basis = capi.gen_lp(2, 4, 10)
    p = ctx.batched_problem(A[None], b[None], c[None], basis[None], True, 6)
    with pytest.raises(capi.LPError):
        p.mip(np.zeros(10, np.int32))
    p.free()
