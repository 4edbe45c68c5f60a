"""Branch-and-bound over variable bounds on the GPU (lp_mip_bounded_solve, lp_mip_bounded_solve_batched): status, found,
x, obj, bound and the five counters equal tests/ref/mip_bounded_ref.c's bit for bit (NaN positions compared, payloads
not) on five shapes and both senses and block sizes, on a 4096-problem batch, on 64 problems of 64 x 192 at depth 64, on
a batch that reaches every outcome, past level 64, with root_status, through the basis=None chain, against
lp_simplex_bounded_resolve_batched for a zero mask, and one problem against a batch of one."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_ref as B
from tests import mip_bounded_ref as R
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


def _skipped(row, status, no):
    """What an LP that root_status keeps out of the search gets."""
    assert row["status"] == status and row["found"] == 0
    assert np.isnan(row["obj"]) and np.isnan(row["bound"]) and np.all(np.isnan(row["x"])) and len(row["x"]) == no
    assert tuple(int(v) for v in row["stats"]) == (0, 0, 0, 0, 0)


def _stack(cases):
    return [np.stack([cs[i] for cs in cases]) for i in range(len(cases[0]))]


@pytest.mark.parametrize("m,n,depth,kind", [(4, 10, 16, "mixed"), (8, 20, 32, "mixed"), (16, 40, 64, "box"),
                                            (32, 96, 256, "box"), (64, 192, 64, "box")])
@pytest.mark.parametrize("maximize", [True, False])
def test_shapes_both_senses_and_block_sizes(ctx, m, n, depth, kind, maximize):
    # (64, 192): 65 x 193 > 4096, sixteen waves; the others four
    assert ctx.mip_bounded_fits(m, n, depth)
    no = n - m
    searched = 0
    for seed in range(3):
        for every in (1, 2):
            A, b, c, lo, hi, mask, _ = R.boxed_mip(seed, m, n, maximize, kind, every)
            root = B.bounded(A, b, c, lo, hi, maximize)
            if root["status"] != OPTIMAL:
                continue
            kw = dict(max_depth=depth, max_nodes=150)
            r = R.mip(A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, no, **kw)
            g = ctx.mip_bounded_solve(A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, no, **kw)
            _same(g, r)
            searched += r["stats"][0] > 1
    assert searched > 0


def _box_batch(B_, m, n, seed0=0):
    cases = [R.boxed_mip(seed0 + k, m, n, True, "box")[:5] for k in range(B_)]
    mask = R.boxed_mip(seed0, m, n, True, "box")[5]
    return _stack(cases) + [mask]


def test_batch_of_4096(ctx):
    Bn, m, n = 4096, 16, 40
    A, b, c, lo, hi, mask = _box_batch(Bn, m, n)
    cold = ctx.bounded_batched(A, b, c, lo, hi, True, n - m)
    assert np.all(cold["status"] == OPTIMAL)
    kw = dict(max_depth=64, max_nodes=60)
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, cold["basis"], cold["at_upper"], maximize=True,
                                        n_orig=n - m, **kw)
    for k in range(Bn):
        r = R.mip(A[k], b[k], c[k], lo[k], hi[k], cold["basis"][k], cold["at_upper"][k], mask, True, n - m, **kw)
        _same(_row(out, k), r)
    assert np.any(out["stats"][:, 0] == 60) and np.any(out["status"] == OPTIMAL)


def test_64_problems_of_64x192_at_depth_64(ctx):
    Bn, m, n = 64, 64, 192
    A, b, c, lo, hi, mask = _box_batch(Bn, m, n, seed0=100)
    cold = ctx.bounded_batched(A, b, c, lo, hi, True, n - m)
    assert np.all(cold["status"] == OPTIMAL)
    kw = dict(max_depth=64, max_nodes=40)
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, cold["basis"], cold["at_upper"], maximize=True,
                                        n_orig=n - m, **kw)
    for k in range(Bn):
        r = R.mip(A[k], b[k], c[k], lo[k], hi[k], cold["basis"][k], cold["at_upper"][k], mask, True, n - m, **kw)
        _same(_row(out, k), r)
    assert out["stats"][:, 4].max() > 8


def _outcome_cases():
    """3 x 7 problems ([A0 | I], 4 integer columns) and the limits max_depth 4, max_nodes 20, max_iter 4 under which
    the reference reaches every outcome; returns (A, b, c, lo, hi, basis, at_upper, mask, kinds, limits, expect)."""
    kw = dict(max_depth=4, max_nodes=20, max_iter=4)
    mask = np.r_[np.ones(4), np.zeros(3)].astype(np.int32)
    I3, slack = np.eye(3), np.array([4, 5, 6], np.int32)
    zero, inf, none = np.zeros(7), np.full(7, np.inf), np.zeros(7, np.int32)
    box = np.r_[np.full(4, 4.0), np.full(3, np.inf)]
    ones = np.hstack([np.ones((3, 4)), I3])
    cases = {
        # 2 x0 + 2 x1 = 1: no integer point, the relaxation feasible
        "integer_infeasible": (np.array([[2.0, 2, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 1, 0], [0, 0, 1, 1, 0, 0, 1]]),
                               np.array([1.0, 5, 3]), np.array([1.0, 1, 1, 1, 0, 0, 0]), zero, box,
                               np.array([0, 5, 6], np.int32), none),
        # column 0 has no positive entry, no upper bound and c_0 > 0
        "unbounded_root": (np.hstack([-np.ones((3, 1)), np.ones((3, 3)), I3]), np.array([2.0, 3, 4]),
                           np.array([1.0, 1, 1, 1, 0, 0, 0]), zero, inf, slack, none),
        # a repeated basis column
        "singular_start": (ones, np.array([2.0, 3, 4]), np.array([1.0, 2, 1, 3, 0, 0, 0]), zero, box,
                           np.array([4, 4, 6], np.int32), none),
        # b_0 < 0 and improving costs: the slack basis is neither primal nor dual feasible
        "no_valid_start": (ones, np.array([-1.0, 3, 3]), np.array([1.0, 2, 1, 3, 0, 0, 0]), zero, box, slack, none),
        # hi_1 < lo_1
        "crossed_bounds": (ones, np.array([2.0, 3, 4]), np.array([1.0, 2, 1, 3, 0, 0, 0]), np.r_[0.0, 2, 0, 0, 0, 0, 0],
                           np.r_[4.0, 1, 4, 4, inf[:3]], slack, none),
    }
    expect = dict(integer_infeasible=INFEASIBLE, unbounded_root=UNBOUNDED, singular_start=SINGULAR,
                  no_valid_start=BAD_ARG, crossed_bounds=INFEASIBLE, optimal=OPTIMAL, node_limit=ITER_LIMIT,
                  depth_limit=ITER_LIMIT, iter_limit=ITER_LIMIT)
    want = ("optimal", "node_limit", "depth_limit", "iter_limit")
    for s in range(4000):
        if all(k in cases for k in want):
            break
        A, b, c, bs, _ = M.knapsack(7000 + s, 3, 4, box=4)
        r = R.mip(A, b, c, zero, box, bs, none, mask, True, 4, **kw)
        st, nodes = r["status"], r["stats"][0]
        if st == OPTIMAL and nodes > 1:
            kind = "optimal"
        elif st == ITER_LIMIT and nodes == kw["max_nodes"]:
            kind = "node_limit"
        elif st == ITER_LIMIT and nodes == 1:
            kind = "iter_limit"
        elif st == ITER_LIMIT and r["found"] and r["bound"] > r["obj"] and r["stats"][4] == kw["max_depth"]:
            kind = "depth_limit"
        else:
            continue
        cases.setdefault(kind, (A, b, c, zero, box, bs, none))
    kinds = sorted(cases)
    return _stack([cases[k] for k in kinds]) + [mask, kinds, kw, expect]


def test_every_outcome_in_one_batch(ctx):
    A, b, c, lo, hi, basis, up, mask, kinds, kw, expect = _outcome_cases()
    assert len(kinds) == 9, kinds
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, maximize=True, n_orig=4, **kw)
    for k, kind in enumerate(kinds):
        r = R.mip(A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, 4, **kw)
        assert r["status"] == expect[kind], kind
        _same(_row(out, k), r)
    dl = _row(out, kinds.index("depth_limit"))
    assert dl["bound"] > dl["obj"]
    assert _row(out, kinds.index("integer_infeasible"))["stats"][0] > 1
    # the single entry raises for the start that is no valid one and returns the other statuses
    k = kinds.index("no_valid_start")
    with pytest.raises(capi.LPError):
        ctx.mip_bounded_solve(A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, 4, **kw)


def test_search_past_level_64(ctx):
    A, b, c, lo, hi, mask, maximize, root = R.deep_case()
    k = R.DEEP_K
    r = R.mip(A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, k, max_depth=1024)
    g = ctx.mip_bounded_solve(A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, k, max_depth=1024)
    _same(g, r)
    assert g["status"] == OPTIMAL and g["stats"][4] > 64


def _small_batch(Bn=12, m=8, n=20, kind="mixed"):
    cases, mask = [], None
    for k in range(Bn):
        A, b, c, lo, hi, mask, _ = R.boxed_mip(40 + k, m, n, True, kind, 2)
        cases.append((A, b, c, lo, hi))
    return _stack(cases) + [mask]


def test_root_status_skips(ctx):
    m, n = 8, 20
    A, b, c, lo, hi, mask = _small_batch()
    cold = ctx.bounded_batched(A, b, c, lo, hi, True, n - m)
    ok = cold["status"] == OPTIMAL
    assert ok.sum() >= 6
    root_status = cold["status"].copy()
    root_status[np.flatnonzero(ok)[1]] = UNBOUNDED   # two solvable LPs kept out by their entries
    root_status[np.flatnonzero(ok)[3]] = ITER_LIMIT
    basis = np.where(ok[:, None], cold["basis"], 0)
    up = np.where(ok[:, None], cold["at_upper"], 0)
    kw = dict(max_depth=32, max_nodes=200)
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, root_status, True, n - m, **kw)
    for k in range(len(A)):
        if root_status[k] != OPTIMAL:
            _skipped(_row(out, k), root_status[k], n - m)
        else:
            _same(_row(out, k), R.mip(A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, n - m, **kw))


def test_chain_from_a_cold_solve(ctx):
    m, n = 8, 20
    A, b, c, lo, hi, mask = _small_batch()
    # one LP made infeasible: a structural column fixed far above what the rows allow
    lo[2, 0] = hi[2, 0] = np.ceil(10.0 * b[2].max() / A[2, :, 0].min())
    kw = dict(max_depth=32, max_nodes=200)
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, maximize=True, n_orig=n - m, **kw)
    cold = ctx.bounded_batched(A, b, c, lo, hi, True, n - m)
    assert cold["status"][2] == INFEASIBLE and (cold["status"] == OPTIMAL).sum() >= 6
    for k in range(len(A)):
        if cold["status"][k] != OPTIMAL:
            _skipped(_row(out, k), cold["status"][k], n - m)
        else:
            _same(_row(out, k), R.mip(A[k], b[k], c[k], lo[k], hi[k], cold["basis"][k], cold["at_upper"][k], mask,
                                      True, n - m, **kw))


@pytest.mark.parametrize("kind", ["bound", "cost"])
def test_zero_mask_is_the_bounded_resolve(ctx, kind):
    """bound: the starts become dual feasible only (the dual loop); cost: primal feasible only (the primal loop and its
    flips).  With the real mask the same starts are searched and compared with the reference."""
    from tests import bounded_resolve_ref as BR
    m, n = 8, 20
    A, b, c, lo, hi, mask = _small_batch()
    cold = ctx.bounded_batched(A, b, c, lo, hi, True, n - m)
    keep = np.flatnonzero(cold["status"] == OPTIMAL)
    A, b, c, lo, hi = A[keep], b[keep], c[keep].copy(), lo[keep].copy(), hi[keep].copy()
    basis, up = cold["basis"][keep], cold["at_upper"][keep]
    full = ctx.bounded_batched(A, b, c, lo, hi, True, n)["x"]
    for k in range(len(keep)):
        _, c[k], lo[k], hi[k] = BR.perturb(k, kind, b[k], c[k], lo[k], hi[k], basis[k], full[k])
    for j in np.flatnonzero(mask):   # (a changed bound of a marked column stays an integer)
        lo[:, j] = np.floor(lo[:, j])
        hi[:, j] = np.where(np.isfinite(hi[:, j]), np.ceil(hi[:, j]), hi[:, j])
    g = ctx.bounded_resolve_batched(A, b, c, lo, hi, basis, up, True, n - m)
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, np.zeros(n, np.int32), basis, up, maximize=True, n_orig=n - m)
    assert np.array_equal(out["status"], g["status"])
    assert np.array_equal(out["stats"][:, 1:4], g["iters"])
    assert np.all(out["stats"][:, 0] == 1) and np.all(out["stats"][:, 4] == 0)
    assert g["iters"][:, 0 if kind == "bound" else 1].sum() > 0
    opt = g["status"] == OPTIMAL
    assert opt.any() and np.array_equal(out["found"], opt.astype(np.int32))
    _bits_equal(out["x"][opt], g["x"][opt])
    _bits_equal(out["obj"][opt], g["obj"][opt])
    assert np.all(np.isnan(out["x"][~opt])) and np.all(np.isnan(out["obj"][~opt]))
    kw = dict(max_depth=32, max_nodes=200)
    srch = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, maximize=True, n_orig=n - m, **kw)
    for k in range(len(keep)):
        _same(_row(srch, k), R.mip(A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, n - m, **kw))


def test_one_problem_equals_a_batch_of_one(ctx):
    m, n = 8, 20
    A, b, c, lo, hi, mask = _small_batch(6)
    cold = ctx.bounded_batched(A, b, c, lo, hi, True, n - m)
    kw = dict(max_depth=32, max_nodes=200)
    done = 0
    for k in np.flatnonzero(cold["status"] == OPTIMAL):
        bs, up = cold["basis"][k], cold["at_upper"][k]
        one = ctx.mip_bounded_solve(A[k], b[k], c[k], lo[k], hi[k], bs, up, mask, True, n - m, **kw)
        b1 = ctx.mip_bounded_solve_batched(A[k:k + 1], b[k:k + 1], c[k:k + 1], lo[k:k + 1], hi[k:k + 1], mask,
                                           bs[None], up[None], maximize=True, n_orig=n - m, **kw)
        r = R.mip(A[k], b[k], c[k], lo[k], hi[k], bs, up, mask, True, n - m, **kw)
        _same(one, r)
        _same(_row(b1, 0), r)
        done += 1
    assert done >= 3


def test_refusals(ctx):
    A, b, c, lo, hi, mask, root = R.boxed_knapsack(0, 3, 5)
    args = (A, b, c, lo, hi, root["basis"], root["at_upper"], mask, True, 5)
    assert ctx.mip_bounded_solve(*args)["status"] == OPTIMAL
    frac = hi.copy()
    frac[0] += 0.5
    for bad in (dict(max_depth=1025), dict(max_depth=-1), dict(max_nodes=0), dict(int_tol=0.5), dict(gap=-1.0),
                dict(eps=-1.0)):
        with pytest.raises(capi.LPError):
            ctx.mip_bounded_solve(*args, **bad)
    with pytest.raises(capi.LPError):
        ctx.mip_bounded_solve(A, b, c, lo, frac, root["basis"], root["at_upper"], mask, True, 5)
    with pytest.raises(capi.LPError):   # a fractional bound in one LP refuses the whole batch
        ctx.mip_bounded_solve_batched(np.stack([A, A]), np.stack([b, b]), np.stack([c, c]), np.stack([lo, lo]),
                                      np.stack([hi, frac]), mask, np.stack([root["basis"]] * 2),
                                      np.stack([root["at_upper"]] * 2), maximize=True, n_orig=5)
    m, n = 160, 320
    assert not ctx.mip_bounded_fits(m, n, 0)
    Ab, bb, cb, basis = capi.gen_lp(0, m, n)
    with pytest.raises(capi.LPError):
        ctx.mip_bounded_solve(Ab, bb, cb, np.zeros(n), np.full(n, np.inf), basis, np.zeros(n, np.int32),
                              np.zeros(n, np.int32), True, n - m, max_depth=0)
