"""The bound-flipping ratio test in the branch-and-bound over the bounds on the GPU: lp_mip_bounded_solve_ratio_ex, its
_batched form and lp_mip_bounded_solve_large_ratio_ex.  Under LP_DUAL_RATIO_LONG_STEP status, found, x, obj, bound and
every counter equal tests/ref/mip_bounded_long_step_ref.c's bit for bit (NaN positions compared, payloads not): in LDS on
five shapes, both senses and both block sizes, on a batch of 64, on the nine-outcome batch, with root_status, through
the basis=None chain, past level 64 and one problem against a batch of one; in HBM at the LDS shapes with no snapshot,
two and one per level, at an odd row length (67 x 201) and beyond the LDS fit at 160 x 320.  LP_DUAL_RATIO_TEXTBOOK through
each new entry equals the old entry in every output, and an unknown ratio is refused with the outputs untouched.
tests/test_mip_bounded_long_step_cpu.py shows on the reference alone that these inputs reach what is claimed."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import mip_bounded_long_step_cases as LC
from tests.test_gpu_mip_bounded import _row, _same, _skipped, _small_batch

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
LONG = dict(dual_ratio="long_step")


def _ref(key, args, K=0, **kw):
    return LC.ref(key, args, dual_ratio=LC.LONG_STEP, snapshots=K, **kw)


def _five(r):
    return dict(r, stats=r["stats"][:5])


def _plain(g):
    return dict(g, stats=tuple(int(v) for v in g["stats"]))


@pytest.mark.parametrize("m,n,depth,kind", LC.LDS_SHAPES)
@pytest.mark.parametrize("maximize", [True, False])
def test_lds_single_and_batched(ctx, m, n, depth, kind, maximize):
    # (64, 192): 65 x 193 > 4096, the 1024-thread form; the others the 256-thread one
    assert ctx.mip_bounded_fits(m, n, depth)
    kw = dict(max_depth=depth, max_nodes=LC.LDS_NODES)
    keys = [(m, n, seed, maximize, kind, 1) for seed in LC.LDS_SEEDS]
    got = [(key, LC.args_of(key)) for key in keys]
    got = [(key, a) for key, a in got if a is not None]
    flipped = 0
    for key, a in got:
        r = _ref(key, a, **kw)
        _same(ctx.mip_bounded_solve(*a, **kw, **LONG), _five(r))
        flipped += r["stats"][0] > 1 and r["stats"][3] > 0
    assert flipped > 0
    A, b, c, lo, hi, basis, up = (np.stack([a[i] for _, a in got]) for i in range(7))
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, got[0][1][7], basis, up, maximize=maximize, n_orig=n - m,
                                        dual_ratio=capi.DUAL_RATIO_LONG_STEP, **kw)
    for k, (key, a) in enumerate(got):
        _same(_row(out, k), _five(_ref(key, a, **kw)))


def test_batch_of_64_row_by_row(ctx):
    (A, b, c, lo, hi, mask, basis, up, status), kw = LC.batch_of_64()
    m, n = A.shape[1:]
    assert np.all(status == OPTIMAL)
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, maximize=True, n_orig=n - m, **kw, **LONG)
    for k in range(len(A)):
        args = (A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, n - m)
        _same(_row(out, k), _five(_ref(("batch64", k), args, **kw)))
    assert out["stats"][:, 3].min() > 0 and np.any(out["stats"][:, 0] == kw["max_nodes"])


def test_every_outcome_in_one_batch(ctx):
    A, b, c, lo, hi, basis, up, mask, kinds, kw, expect = LC.outcome_cases()
    assert len(kinds) == 9, kinds
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, maximize=True, n_orig=4, **kw, **LONG)
    for k, kind in enumerate(kinds):
        args = (A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, 4)
        r = _ref(("outcome", kind), args, **kw)
        assert r["status"] == expect[kind], kind
        _same(_row(out, k), _five(r))
    assert out["stats"][:, 3].sum() > 0
    k = kinds.index("no_valid_start")
    with pytest.raises(capi.LPError):
        ctx.mip_bounded_solve(A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, 4, **kw, **LONG)


def test_root_status_and_the_chain_from_a_cold_solve(ctx):
    m, n = 8, 20
    A, b, c, lo, hi, mask = _small_batch()
    lo[2, 0] = hi[2, 0] = np.ceil(10.0 * b[2].max() / A[2, :, 0].min())   # one LP made infeasible
    kw = dict(max_depth=32, max_nodes=200)
    cold = ctx.bounded_batched(A, b, c, lo, hi, True, n - m)
    ok = cold["status"] == OPTIMAL
    assert cold["status"][2] == INFEASIBLE and ok.sum() >= 6
    chain = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, maximize=True, n_orig=n - m, **kw, **LONG)
    root_status = cold["status"].copy()
    root_status[np.flatnonzero(ok)[1]] = UNBOUNDED   # a solvable LP kept out by its entry
    basis = np.where(ok[:, None], cold["basis"], 0)
    up = np.where(ok[:, None], cold["at_upper"], 0)
    kept = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, root_status, True, n - m, **kw, **LONG)
    flips = 0
    for k in range(len(A)):
        args = (A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, n - m)
        if cold["status"][k] != OPTIMAL:
            _skipped(_row(chain, k), cold["status"][k], n - m)
        else:
            r = _five(_ref(("small", k), args, **kw))
            _same(_row(chain, k), r)
            flips += r["stats"][3]
        if root_status[k] != OPTIMAL:
            _skipped(_row(kept, k), root_status[k], n - m)
        else:
            _same(_row(kept, k), _five(_ref(("small", k), args, **kw)))
    assert flips > 0


def test_search_past_level_64(ctx):
    args, kw = LC.deep_args()
    r = _ref(("deep",), args, **kw)
    g = ctx.mip_bounded_solve(*args, **kw, **LONG)
    _same(g, _five(r))
    assert g["status"] == OPTIMAL and g["stats"][4] > 64 and g["stats"][3] > 0


def test_one_problem_equals_a_batch_of_one(ctx):
    key, args, kw = LC.root_after_bound_change()
    r = _five(_ref(key, args, **kw))
    one = ctx.mip_bounded_solve(*args, **kw, **LONG)
    A, b, c, lo, hi, basis, up, mask, mx, no = args
    b1 = ctx.mip_bounded_solve_batched(A[None], b[None], c[None], lo[None], hi[None], mask, basis[None], up[None],
                                       maximize=mx, n_orig=no, **kw, **LONG)
    _same(one, r)
    _same(_row(b1, 0), r)
    assert r["stats"][3] > 0


def test_a_node_at_max_iter(ctx):
    for key, args, kw in LC.node_at_max_iter():
        r = _ref(key, args, **kw)
        assert r["status"] == ITER_LIMIT
        _same(ctx.mip_bounded_solve(*args, **kw, **LONG), _five(r))
        for K in (0, 2):
            _same(ctx.mip_bounded_solve_large(*args, snapshots=K, **kw, **LONG), _ref(key, args, K, **kw))


@pytest.mark.parametrize("m,n,depth,kind", LC.LDS_SHAPES)
def test_hbm_entry_at_the_lds_shapes(ctx, m, n, depth, kind):
    kw = dict(max_depth=depth, max_nodes=LC.LDS_NODES)
    restored = flips = 0
    for maximize in (True, False):
        key = (m, n, 1, maximize, kind, 1)
        args = LC.args_of(key)
        lds = ctx.mip_bounded_solve(*args, **kw, **LONG)
        for K in LC.LDS_KS + (depth,):
            g = ctx.mip_bounded_solve_large(*args, snapshots=K, **kw, **LONG)
            _same(g, _ref(key, args, K, **kw))
            if K == 0:
                _same(_five(_plain(g)), _plain(lds))
            restored += g["stats"][5]
            flips += g["stats"][3]
    assert restored > 0 and flips > 0


_BEYOND = [(key, kw) for key, kw in LC.beyond_keys() if key[2] in (1, 3)]


@pytest.mark.parametrize("key,kw", _BEYOND, ids=["-".join(map(str, k)) for k, _ in _BEYOND])
def test_beyond_the_lds_fit(ctx, key, kw):
    # 160 x 320 is beyond lp_mip_bounded_fits; 67 x 201 (202 columns padded to 208 in HBM) also runs in LDS
    lds = ctx.mip_bounded_fits(key[0], key[1], kw["max_depth"])
    assert lds == (key[0] == 67)
    args = LC.args_of(key)
    for K in LC.BEYOND_KS:
        g = ctx.mip_bounded_solve_large(*args, snapshots=K, **kw, **LONG)
        _same(g, _ref(key, args, K, **kw))
        assert g["stats"][3] > 0 and (K == 0 or g["stats"][5] > 0)
        if lds and K == 0:
            _same(_five(_plain(g)), _plain(ctx.mip_bounded_solve(*args, **kw, **LONG)))


def test_textbook_through_the_new_entries_is_the_old_entry(ctx):
    key, args, kw = LC.root_after_bound_change()
    old = ctx.mip_bounded_solve(*args, **kw)
    _same(ctx.mip_bounded_solve(*args, **kw, dual_ratio="textbook"), _plain(old))
    assert old["stats"][0] > 1 and old["stats"][3] == 0
    A, b, c, lo, hi, basis, up, mask, mx, no = args
    batch = [A[None], b[None], c[None], lo[None], hi[None], mask, basis[None], up[None]]
    oldb = ctx.mip_bounded_solve_batched(*batch, maximize=mx, n_orig=no, **kw)
    newb = ctx.mip_bounded_solve_batched(*batch, maximize=mx, n_orig=no, **kw, dual_ratio=capi.DUAL_RATIO_TEXTBOOK)
    _same(_row(newb, 0), _plain(_row(oldb, 0)))
    for K in (0, 2):
        oldl = ctx.mip_bounded_solve_large(*args, snapshots=K, **kw)
        _same(ctx.mip_bounded_solve_large(*args, snapshots=K, **kw, dual_ratio="textbook"), _plain(oldl))
    five = ctx.mip_bounded_solve_large(*args, **kw, dual_ratio="textbook")
    assert len(five["stats"]) == 5
    _same(five, _plain(ctx.mip_bounded_solve_large(*args, **kw)))
    bkey, bkw = _BEYOND[0]
    bargs = LC.args_of(bkey)
    _same(ctx.mip_bounded_solve_large(*bargs, snapshots=4, **bkw, dual_ratio="textbook"),
          _plain(ctx.mip_bounded_solve_large(*bargs, snapshots=4, **bkw)))


@pytest.mark.parametrize("dual_ratio", [2, -1])
def test_an_unknown_ratio_is_refused_and_writes_nothing(ctx, dual_ratio):
    key, args, kw = LC.root_after_bound_change()
    for call in (ctx.mip_bounded_solve, ctx.mip_bounded_solve_large):
        with pytest.raises(capi.LPError) as e:
            call(*args, **kw, dual_ratio=dual_ratio)
        assert e.value.code == BAD_ARG
    A, b, c, lo, hi, basis, up, mask, mx, no = args
    with pytest.raises(capi.LPError):
        ctx.mip_bounded_solve_batched(A[None], b[None], c[None], lo[None], hi[None], mask, basis[None], up[None],
                                      maximize=mx, n_orig=no, dual_ratio=dual_ratio, **kw)
    # through ctypes: the output arrays passed in keep their contents (ahead of every other check: a bad basis, a
    # negative eps and a bad snapshot count ride along)
    m, n = A.shape
    Af = capi.colmajor(A)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    d = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    i = lambda a: a.ctypes.data_as(ip)   # noqa: E731
    keep = [np.ascontiguousarray(v, np.float64) for v in (b, c, lo, hi)]
    bad_basis = np.full(m, -7, np.int32)
    upi, maski = np.ascontiguousarray(up, np.int32), np.ascontiguousarray(mask, np.int32)
    x, obj, bound = np.full(no, 7.0), np.full(1, 7.0), np.full(1, 7.0)
    found, stats, st = np.full(1, 7, np.int32), np.full(7, 7, np.int32), np.full(1, 7, np.int32)
    head = (d(Af), m, n, d(keep[0]), d(keep[1]), d(keep[2]), d(keep[3]), i(bad_basis), i(upi))
    tail = (int(mx), no, i(maski), -1.0, 1e-6, 1e-9, 8, 10, 100, d(x), d(obj), d(bound), i(found), i(stats))
    lib = ctx.lib
    assert lib.lp_mip_bounded_solve_ratio_ex(ctx.h, *head, *tail, dual_ratio) == BAD_ARG
    assert lib.lp_mip_bounded_solve_large_ratio_ex(ctx.h, *head, *tail, -3, dual_ratio) == BAD_ARG
    assert lib.lp_mip_bounded_solve_batched_ratio_ex(ctx.h, 1, *head, None, *tail, i(st), dual_ratio) == BAD_ARG
    assert np.all(x == 7.0) and obj[0] == 7.0 and bound[0] == 7.0
    assert found[0] == 7 and np.all(stats == 7) and st[0] == 7
    # the context stays usable
    _same(ctx.mip_bounded_solve(*args, **kw, **LONG), _five(_ref(key, args, **kw)))
