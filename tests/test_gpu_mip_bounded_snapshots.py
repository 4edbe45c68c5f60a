"""Branch-and-bound beyond LDS with tableau snapshots (lp_mip_bounded_solve_large_ex): status, found, x, obj, bound and
all seven counters equal tests/ref/mip_bounded_snapshots_ref.c's bit for bit (NaN positions compared, payloads not): on
4 x 14 knapsacks with one slot, a small ring and a slot per level (restores, ring overwrites with rebuilds, restored
children that end infeasible), at a shape that also fits LDS, at an odd row length, at 160 x 320, with no snapshot
against the entry without the argument, at every stopping rule, with more rows than a block has threads (against a
recorded reference result), and after a refused call.  tests/test_mip_bounded_snapshots_cpu.py shows on the reference
alone that these inputs reach what is claimed for them."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import mip_bounded_large_cases as Q
from tests import mip_bounded_snapshots_cases as SC
from tests.test_gpu_mip_bounded import _same

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def _plain(g):
    return dict(g, stats=tuple(int(v) for v in g["stats"]))


@pytest.mark.parametrize("seed", sorted(SC.KNAP_AT_3))
@pytest.mark.parametrize("K", SC.KNAP_KS)
def test_knapsacks(ctx, seed, K):
    args = SC.knapsack_args(seed)
    r = SC.ref(("knap", seed), args, snapshots=K, **SC.KNAP_KW)
    g = ctx.mip_bounded_solve_large(*args, snapshots=K, **SC.KNAP_KW)
    _same(g, r)
    assert g["stats"][5] > 0 and (K == 24) == (g["stats"][6] == 0)


@pytest.mark.parametrize("maximize", [True, False])
def test_a_shape_that_also_fits_lds(ctx, maximize):
    m, n, depth, kind = SC.LDS_BOX
    assert ctx.mip_bounded_fits(m, n, depth)
    kw = dict(max_depth=depth, max_nodes=Q.LDS_NODES)
    restored = 0
    for seed in range(3):
        for every in (1, 2):
            got = Q.searched(m, n, seed, maximize, kind, every, **kw)
            if got is None:
                continue
            args = got[0]
            key = (m, n, seed, maximize, kind, every)
            for K in SC.KS_LDS_BOX:
                g = ctx.mip_bounded_solve_large(*args, snapshots=K, **kw)
                _same(g, SC.ref(key, args, snapshots=K, **kw))
                restored += g["stats"][5]
            g0 = ctx.mip_bounded_solve_large(*args, snapshots=0, **kw)
            _same(g0, SC.ref(key, args, snapshots=0, **kw))
            _same(dict(g0, stats=g0["stats"][:5]), _plain(ctx.mip_bounded_solve(*args, **kw)))
    assert restored > 0


@pytest.mark.parametrize("key,kw,Ks", SC.gpu_keys(), ids=["-".join(map(str, k[0])) for k in SC.gpu_keys()])
def test_beyond_the_lds_fit(ctx, key, kw, Ks):
    args = Q.searched(*key, **kw)[0]
    for K in Ks:
        g = ctx.mip_bounded_solve_large(*args, snapshots=K, **kw)
        _same(g, SC.ref(key, args, snapshots=K, **kw))
        assert g["stats"][5] > 0


def test_no_snapshot_is_the_entry_without_the_argument(ctx):
    cases = [(("knap", 1), SC.knapsack_args(1), SC.KNAP_KW)]
    for key, args, kw, _ in SC.gpu_cases():
        if key in ((67, 201, 1, True, "mixed", 2), (160, 320, 1, True, "box", 1)):
            cases.append((key, args, kw))
    assert len(cases) == 3
    for key, args, kw in cases:
        g0 = ctx.mip_bounded_solve_large(*args, snapshots=0, **kw)
        old = ctx.mip_bounded_solve_large(*args, **kw)
        assert len(old["stats"]) == 5 and len(g0["stats"]) == 7
        _same(dict(g0, stats=g0["stats"][:5]), _plain(old))
        _same(g0, SC.ref(key, args, snapshots=0, **kw))
        assert g0["stats"][5] == 0 and g0["stats"][6] > 0


def test_stopping_rules(ctx):
    args = SC.knapsack_args(1)
    for kind, N in sorted(SC.stop_points(1, 3).items()):
        kw = dict(max_depth=SC.KNAP_KW["max_depth"], max_nodes=N)
        g = ctx.mip_bounded_solve_large(*args, snapshots=3, **kw)
        _same(g, SC.ref(("knap", 1), args, snapshots=3, **kw))
        assert g["status"] == ITER_LIMIT and g["stats"][0] == N, kind
    # a restored child that ends LP_ITER_LIMIT stops the search with that status; so does the rebuilt one
    args, kw = SC.iter_limit_case()
    for K in (3, 0):
        g = ctx.mip_bounded_solve_large(*args, snapshots=K, **kw)
        _same(g, SC.ref(("iter-limit",), args, snapshots=K, **kw))
        assert g["status"] == ITER_LIMIT and g["stats"][5] == (1 if K else 0)


def test_more_rows_than_a_block_has_threads(ctx):
    m, n = Q.TALL_SHAPE
    assert m > 1024
    want, _ = SC.tall_fixture()
    g = ctx.mip_bounded_solve_large(*Q.tall_args(1), max_depth=SC.TALL_DEPTH, max_nodes=SC.TALL_NODES,
                                    max_iter=Q.TALL_MAX_ITER, snapshots=SC.TALL_SNAPSHOTS)
    _same(g, want)
    assert g["stats"][5] == 2


def test_refusals_leave_the_context_usable_and_no_slot_state_leaks(ctx):
    args = SC.knapsack_args(2)
    for bad in (dict(snapshots=-1), dict(snapshots=1025), dict(snapshots=3, max_depth=1025),
                dict(snapshots=3, max_nodes=0), dict(snapshots=3, int_tol=0.5), dict(snapshots=3, eps=-1.0)):
        with pytest.raises(capi.LPError):
            ctx.mip_bounded_solve_large(*args, **dict(SC.KNAP_KW, **bad))
    # through the raw symbol: LP_BAD_ARG, nothing launched and no output written
    A, b, c, lo, hi, basis, up, mask, maximize, n_orig = args
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c, lo, hi = (np.ascontiguousarray(v, np.float64) for v in (b, c, lo, hi))
    basis, up, mask = (np.ascontiguousarray(v, np.int32) for v in (basis, up, mask))
    d, i = capi._d, capi._i
    x, obj, bound = np.full(n_orig, 7.0), np.full(1, 7.0), np.full(1, 7.0)
    found, stats = np.full(1, 7, np.int32), np.full(7, 7, np.int32)
    good = [ctx.h, d(Af), 4, 14, d(b), d(c), d(lo), d(hi), i(basis), i(up), 1, n_orig, i(mask), 1e-9, 1e-6, 1e-9, 24, 400,
            10000, d(x), d(obj), d(bound), i(found), i(stats), 3]
    for pos, value in ((24, -1), (24, 1025), (16, 1025), (17, 0), (14, 0.5), (13, -1.0), (11, 0), (22, None)):
        call = list(good)
        call[pos] = value
        assert ctx.lib.lp_mip_bounded_solve_large_ex(*call) == BAD_ARG, pos
        assert np.all(x == 7.0) and obj[0] == bound[0] == 7.0 and found[0] == 7 and np.all(stats == 7), pos
    with pytest.raises(capi.LPError):
        ctx.mip_bounded_snapshot_bytes(4, 14, 1025)
    assert ctx.mip_bounded_snapshot_bytes(4, 14, 3) == 3 * 8 * (5 * 16 + 2 * 14)
    # searches in a row on one context, each with its own ring
    for K in (24, 1, 3, 0, 3):
        _same(ctx.mip_bounded_solve_large(*args, snapshots=K, **SC.KNAP_KW),
              SC.ref(("knap", 2), args, snapshots=K, **SC.KNAP_KW))
