"""The node decisions of the three branch-and-bound kernels at exact ties (tests/mip_tie_cases.py; what each input is
designed to do is asserted without a GPU in tests/test_mip_ties_cpu.py): the branching column among tied dist values
across every seam of the column scans, dist against int_tol, f against 0.5 with floor and ceil of negative values, z
against zstar +- gap in the pruning test, the final status and the final bound, the objective chain past 4096 products
and the branching column at a basis position past 1024.  Every case runs on lp_mip_bounded_solve_large, on
lp_mip_bounded_solve where lp_mip_bounded_fits takes the shape at that depth, and without its boxes on lp_mip_solve
where lp_mip_fits does; the two fits answers are asserted against the literal tables of the case module and nothing else
decides.  status, found, x, obj, bound and the counters equal tests/ref/mip_bounded_ref.c's (tests/ref/mip_ref.c's) bit
for bit, and where a shape runs on both bounded paths the two results are equal.

Flagged basic columns (at_upper = 1 on a basic column, the `if (f)` arms of the dive): the bounded entries accept such
a start, and dir_flagged runs on them.  lp_mip_solve has no flags and no lower bounds: dir_neg, dir_flagged and the
chain do not run there.

Left out: the handle form BatchedProblem.mip, whose run ends at the basis of the solver's own pivoting, not at a
designed one."""
import numpy as np
import pytest

from tests import mip_tie_cases as K
from tests.test_gpu_mip import _same as _same_plain
from tests.test_gpu_mip_bounded import _row, _same

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def _as_ref(g):
    return dict(g, stats=tuple(int(v) for v in g["stats"]))


def _run(ctx, cs, max_depth=K.DEEP, **kw):
    """cs under the limits kw on every entry that takes its shape at max_depth; returns the number of entries run."""
    m, n = cs.shape
    kw = dict(kw, max_depth=max_depth)
    r = K.ref_bounded(cs, **kw)
    g = ctx.mip_bounded_solve_large(*K.bounded_args(cs), **kw)
    _same(g, r)
    ran = 1
    lds = ctx.mip_bounded_fits(m, n, max_depth)
    assert lds == K.fits(K.BOUNDED_FITS_TO, cs.shape, max_depth)
    if lds:
        g2 = ctx.mip_bounded_solve(*K.bounded_args(cs), **kw)
        _same(g2, r)
        _same(g2, _as_ref(g))
        ran += 1
    row_form = ctx.mip_fits(m, n, max_depth)
    assert row_form == K.fits(K.PLAIN_FITS_TO, cs.shape, max_depth)
    if row_form and cs.plain:
        _same_plain(ctx.mip(*K.plain_args(cs), **kw), K.ref_plain(cs, **kw))
        ran += 1
    return ran


# ---- A: the order of tied columns
@pytest.mark.parametrize("name,shape", K.ORDER_CASES)
def test_order_of_tied_columns_at_every_depth(ctx, name, shape):
    cs = K.order_case(name, shape)
    ran = [_run(ctx, cs, d) for d in K.depths(cs)]
    # WIDE: the HBM entry alone; LDS16: the row form up to depth 22; LDS4: all three at every depth
    assert ran == {K.WIDE: [1] * len(ran), K.LDS16: [3] * (len(ran) - 1) + [2], K.LDS4: [3] * len(ran)}[shape]


# ---- B: dist against int_tol
@pytest.mark.parametrize("name", sorted(K.TOL_CASES))
def test_int_tol_edge(ctx, name):
    cs = K.tol_case(name)
    assert _run(ctx, cs, **{k: v for k, v in cs.kw.items() if k != "max_depth"}) == (1 if cs.shape == K.WIDE else 3)


# ---- C: direction, negative values, flagged basic columns
@pytest.mark.parametrize("name", sorted(K.DIR_COLS))
def test_directions_at_every_depth_and_node_limit(ctx, name):
    cs = K.dir_case(name)
    entries = 3 if cs.plain else 2
    for d in K.depths(cs):
        assert _run(ctx, cs, d) == entries
    for nodes in K.node_limits(cs):
        assert _run(ctx, cs, max_nodes=nodes) == entries


# ---- D: z against zstar +- gap
@pytest.mark.parametrize("shape", [K.SMALL, K.WIDE])
@pytest.mark.parametrize("maximize", [True, False])
def test_gap_edge(ctx, shape, maximize):
    cs = K.gap_case(shape, maximize)
    for gap in K.GAPS:
        assert _run(ctx, cs, gap=gap) == (1 if shape == K.WIDE else 3)


@pytest.mark.parametrize("shape", [K.SMALL, K.WIDE])
@pytest.mark.parametrize("maximize", [True, False])
def test_gap_edge_at_the_depth_limit(ctx, shape, maximize):
    cs = K.gap_case(shape, maximize, y_marked=True)
    for gap in K.GAPS:
        assert _run(ctx, cs, 1, gap=gap) == (1 if shape == K.WIDE else 3)


@pytest.mark.parametrize("maximize", [True, False])
def test_gap_edge_of_the_final_bound_at_the_node_limit(ctx, maximize):
    cs = K.gap_case(K.SMALL, maximize)
    for gap in K.LIMIT_GAPS:
        assert _run(ctx, cs, gap=gap, max_nodes=2) == 3


def test_two_abandoned_nodes_of_equal_z(ctx):
    assert _run(ctx, K.gap_twin_case(), **K.TWIN_RUN) == 3
    assert _run(ctx, K.gap_twin_case()) == 3


# ---- E: the objective chain across 4096 products
def test_objective_chain_across_4096_products(ctx):
    cs = K.chain_case()
    for d in K.depths(cs):
        assert _run(ctx, cs, d) == 1


# ---- F: the branching column at a basis position >= 1024
def test_branching_column_at_basis_position_1030(ctx):
    cs = K.tall_case()
    want = K.tall_fixture()
    assert (want["status"], want["bound"], want["stats"]) == K.TALL_WANT
    assert not ctx.mip_bounded_fits(*cs.shape, 1) and not ctx.mip_fits(*cs.shape, 1)
    _same(ctx.mip_bounded_solve_large(*K.bounded_args(cs), **K.TALL_RUN), want)


# ---- the batch
def _stack(cases, attrs):
    return [np.stack([getattr(c, a) for c in cases]) for a in attrs]


def test_one_launch_of_different_decisions(ctx):
    cases = K.batch_cases(False)
    A, b, c, lo, hi, basis, up = _stack(cases, ("A", "b", "c", "lo", "hi", "basis", "up"))
    out = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, cases[0].mask, basis, up, maximize=True,
                                        n_orig=cases[0].n_orig, **K.BATCH_KW)
    for k, cs in enumerate(cases):
        r = K.ref_bounded(cs, **K.BATCH_KW)
        _same(_row(out, k), r)
        _same(_as_ref(ctx.mip_bounded_solve(*K.bounded_args(cs), **K.BATCH_KW)), r)
    plain = K.batch_cases(True)
    A, b, c, basis = _stack(plain, ("A", "b", "c", "basis"))
    out = ctx.mip_batched(A, b, c, basis, plain[0].mask, True, plain[0].n_orig, **K.BATCH_KW)
    for k, cs in enumerate(plain):
        r = K.ref_plain(cs, **K.BATCH_KW)
        _same_plain(_row(out, k), r)
        _same_plain(ctx.mip(*K.plain_args(cs), **K.BATCH_KW), r)
