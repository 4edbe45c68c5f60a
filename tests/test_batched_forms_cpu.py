"""CPU-only: the inputs of tests/batched_form_cases.py reach what they are listed for.  lp_batched_form (host
arithmetic, no device) gives every shape the form of the table, the dispatch flips exactly at the listed neighbours,
and on the oracle's traces the leaving rows of each shape's batch touch every row group, every row-in-group index, the
rows from 256 on and the last row in front of the padding; every near-tie pair leaves from its second row at eps = 0
and from its first at 1e-9.  tests/test_gpu_batched_forms.py runs the same batches on the kernels."""
import functools

import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import batched_form_cases as F

IDS = [f"{m}x{n}" for m, n in F.SHAPES]


@functools.lru_cache(maxsize=None)
def _traces(m, n):
    """Per LP of batch(m, n): the oracle's results at F.EPS, with the (entering, leaving row) trace."""
    A, b, c, basis = F.batch(m, n)
    return tuple(tuple(o.simplex_tableau(A[k], b[k], c[k], basis[k], True, n - m, eps=eps, trace_cap=1 << 12)
                       for eps in F.EPS) for k in range(len(A)))


def _form(m, n):
    fits, threads, rpt, aligned, dreg = capi.batched_form(m, n)
    assert fits, (m, n)   # lp_batched_lds_bytes(m, n) <= 160 KiB: the batch runs one LP per workgroup
    return threads, rpt, aligned, dreg


@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_form_table(shape):
    threads, rpt, aligned, dreg, _ = F.FORMS[shape]
    assert _form(*shape) == ((threads, rpt, aligned, dreg) if threads else (0, 0, False, False))


def test_every_form_and_layout_is_listed():
    """The four instantiations, each aligned and with the reduced costs in registers and in LDS, and the LDS form; among the aligned layouts every RX, a single row group, a group of padding only, idle waves behind xB's."""
    cells = {(t, r, a, d) for t, r, a, d, _ in F.FORMS.values()}
    for threads, rpt in ((1024, 4), (1024, 12), (512, 44), (1024, 20)):
        # (the plain layout of 12 rows is tests/test_gpu_rows_beyond_wave.py's 100 x 150)
        assert {a for t, r, a, d in cells if (t, r) == (threads, rpt)} == ({True} if rpt == 12 else {True, False})
        assert {d for t, r, a, d in cells if (t, r) == (threads, rpt)} == {True, False}
    assert (0, 0, False, False) in cells
    geo = {s: F.geometry(*s) for s in F.SHAPES if F.FORMS[s][0]}
    assert {g["RX"] for g in geo.values() if g["aligned"]} == {1, 2, 3, 4}
    assert {(g["aligned"], g["G"]) for g in geo.values()} >= {(True, 1), (False, 1), (True, 2)}
    assert any(g["mp"] - m >= g["rpt"] for (m, _), g in geo.items())
    assert any(g["aligned"] and g["G"] * g["CW"] + 2 < g["threads"] // 64 for g in geo.values())


def test_dispatch_flips_at_the_listed_neighbours():
    for (below, form_below), (above, form_above) in F.FLIPS:
        assert _form(*below)[:2] == form_below, below
        assert _form(*above)[:2] == form_above, above


def test_shapes_that_do_not_fit():
    assert capi.batched_form(8, 8) == (False, 0, 0, False, False)
    assert capi.batched_form(0, 4) == (False, 0, 0, False, False)
    assert capi.batched_form(200, 600) == (False, 0, 0, False, False)   # 201 x 401 doubles: beyond one CU's LDS


@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_every_lp_ends_optimal(shape):
    for name, runs in zip(F.names(*shape), _traces(*shape)):
        for r in runs:
            assert r["status"] == o.OPTIMAL and r["iters"] == len(r["trace"]), name


@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_leaving_rows_reach_the_cell(shape):
    m, n = shape
    rows = {leave for runs in _traces(m, n) for r in runs for _, leave in r["trace"]}
    assert rows and max(rows) < m
    g = F.geometry(m, n)
    if g:
        rpt = g["rpt"]
        assert {r // rpt for r in rows} == {i // rpt for i in range(m)}
        assert {r % rpt for r in rows} == {i % rpt for i in range(m)}
        if g["mp"] > m:
            assert m - 1 in rows
    if m > 256:
        assert max(rows) >= 256 and m - 1 in rows


@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_pairs_flip_with_eps(shape):
    m, n = shape
    pairs = F.pairs(m, n)
    g = F.geometry(m, n)
    if g and m > g["rpt"]:
        assert pairs[0] == (g["rpt"] - 1, g["rpt"])
    assert pairs
    runs = _traces(m, n)
    for k, (p, q) in zip(F.pair_slice(m, n), pairs):
        at_1e9, at_0 = runs[k]
        assert F.EPS == (1e-9, 0.0)
        assert at_1e9["trace"][0][1] == p and at_0["trace"][0][1] == q, (p, q)
        assert at_1e9["trace"][0][0] == at_0["trace"][0][0]


@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_a_limit_stops_some_lps_and_not_others(shape):
    m, n = shape
    counts = [runs[0]["iters"] for runs in _traces(m, n)]
    limit = F.iteration_limit(counts)
    assert min(counts) < limit <= max(counts)   # (an LP that needs exactly `limit` pivots is stopped)
    A, b, c, basis = F.batch(m, n)
    stopped = {o.simplex_tableau(A[k], b[k], c[k], basis[k], True, n - m, max_iter=limit)["status"]
               for k in range(len(A))}
    assert stopped == {o.OPTIMAL, o.ITER_LIMIT}
