"""Batched two-phase simplex (lp_simplex_two_phase_batched, lp_batched_two_phase_upload): every LP of
a batch bit-exact against the oracle's orc_two_phase — status, the three pivot counts and the basis;
for optimal LPs also the vertex and the objective."""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import handlecases, lpcases

pytestmark = pytest.mark.gpu


def _stack(cases):
    A = np.stack([q[0] for q in cases])
    b = np.stack([q[1] for q in cases])
    c = np.stack([q[2] for q in cases])
    return A, b, c


def _oracle(cases, maximize=False, max_iter=capi.MAX_ITER):
    return [o.two_phase(A, b, c, maximize=maximize, n_orig=no, max_iter=max_iter) for A, b, c, no in cases]


def _assert_same(g, refs):
    for k, r in enumerate(refs):
        assert g["status"][k] == r["status"], k
        assert g["iters"][k].tolist() == list(r["iters"]), k
        assert np.array_equal(g["basis"][k], r["basis"]), k
        if r["status"] == o.OPTIMAL:
            assert np.array_equal(g["x"][k], r["x"]), k   # bit for bit
            assert g["obj"][k] == r["obj"], k


def _solve(ctx, cases, maximize=False, max_iter=capi.MAX_ITER, want_path=1):
    """The handle form (checks the path), then the one-shot form; both against each other."""
    A, b, c = _stack(cases)
    no = cases[0][3]
    p = ctx.batched_two_phase_problem(A, b, c, maximize=maximize, n_orig=no)
    try:
        assert p.path() == want_path
        p.run(max_iter=max_iter)
        h = p.download()
        h["iters"] = p.phase_iters()
    finally:
        p.free()
    g = ctx.two_phase_batched(A, b, c, maximize=maximize, n_orig=no, max_iter=max_iter)
    for key in ("status", "iters", "basis", "x", "obj"):
        assert np.array_equal(g[key], h[key], equal_nan=True), key
    return g


@pytest.mark.parametrize("m,k", [(2, 3), (5, 4), (8, 16), (16, 32), (32, 64), (64, 128)])
def test_shapes_mixed_rows(ctx, m, k):
    cases = []
    for seed in range(24):
        eq = seed % (m // 2 + 1)
        neg = (seed // 2) % (m + 1)
        zr = (seed // 3) % (m - eq + 1) if m > 2 else seed % 2
        cases.append(lpcases.min_lp(seed, m, k, equalities=eq, negative_rows=neg, zero_rhs=min(zr, m - eq)))
    refs = _oracle(cases)
    _assert_same(_solve(ctx, cases), refs)


def test_degenerate_drive_out(ctx):
    cases = [lpcases.degenerate_eq_lp(seed) for seed in range(60)]
    refs = _oracle(cases)
    g = _solve(ctx, cases)
    _assert_same(g, refs)
    assert g["iters"][:, 1].sum() > 0   # the drive-out ran on the device


def _le_form(seed, m, k):
    """max c.x, A0 x <= b with slacks: a short phase I and, for some seeds, a long phase II."""
    rng = np.random.default_rng(5000 + seed)
    A = np.hstack([rng.uniform(0, 1, (m, k)), np.eye(m)])
    b = rng.uniform(1, 2, m)
    c = np.concatenate([rng.uniform(0.1, 1, k), np.zeros(m)])
    return A, b, c, k


def test_mixed_outcomes(ctx):
    m, k, limit = 8, 12, 10

    def bounded(seed):   # row m-1 becomes A0 x + s = b: the maximum exists
        A, b, c, no = lpcases.min_lp(seed, m, k)
        A[m - 1, k + m - 1] = 1.0
        return A, b, c, no

    def infeasible(seed):   # A0 x = -1 with A0 >= 0
        A, b, c, no = lpcases.min_lp(seed, m, k)
        A[0, k:] = 0.0
        b[0] = -1.0
        return A, b, c, no

    def singular(seed):   # a duplicated equality row: one artificial cannot leave
        A, b, c, no = lpcases.min_lp(seed, m, k, equalities=2)
        A[1] = A[0]
        b[1] = b[0]
        return A, b, c, no

    cases = ([bounded(s) for s in (0, 1, 2, 3)] + [lpcases.min_lp(s, m, k) for s in (0, 1)] +
             [infeasible(s) for s in (2, 3)] + [singular(s) for s in (0, 1)] + [_le_form(5, m, k)])
    refs = _oracle(cases, maximize=True, max_iter=limit)
    kinds = {(r["status"], r["iters"][2] > 0) if r["status"] == o.ITER_LIMIT else r["status"] for r in refs}
    assert {o.OPTIMAL, o.INFEASIBLE, o.SINGULAR, o.UNBOUNDED, (o.ITER_LIMIT, False), (o.ITER_LIMIT, True)} <= kinds
    _assert_same(_solve(ctx, cases, maximize=True, max_iter=limit), refs)


def test_golden_cases(ctx):
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "two_phase_cases.json")))
    groups = {}
    for g in golden:
        if g["kind"] == "min":
            a = g["args"]
            case = lpcases.min_lp(g["seed"], a[0], a[1], equalities=a[2], negative_rows=a[3], zero_rhs=a[4])
        else:
            case = lpcases.degenerate_eq_lp(g["seed"])
        groups.setdefault((case[0].shape, case[3]), []).append((case, g))
    for items in groups.values():
        r = _solve(ctx, [q[0] for q in items])
        for k, (_, g) in enumerate(items):
            assert r["status"][k] == o.OPTIMAL and r["iters"][k].tolist() == g["iters"]
            assert r["basis"][k].tolist() == g["basis"] and r["obj"][k] == g["obj"] and r["x"][k].tolist() == g["x"]


def test_full_size_4096(ctx):
    cases = [lpcases.min_lp(seed, 64, 128) for seed in range(4096)]
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=128)
    try:
        assert p.path() == 1
        p.run()
        g = p.download()
        g["iters"] = p.phase_iters()
    finally:
        p.free()
    _assert_same(g, _oracle(cases))


def test_shape_beyond_fits_falls_back(ctx):
    cases = [lpcases.min_lp(seed, 128, 128) for seed in range(3)]
    _assert_same(_solve(ctx, cases, want_path=0), _oracle(cases))


def test_handle_rerun_iters_and_shards(ctx):
    cases = [lpcases.min_lp(seed, 16, 32, equalities=seed % 3, negative_rows=seed % 4) for seed in range(40)]
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, n_orig=32)
    try:
        p.run()
        first, it_first = p.download(), p.phase_iters()
        p.run()
        second, it_second = p.download(), p.phase_iters()
    finally:
        p.free()
    for key in ("status", "iters", "basis", "x", "obj"):
        assert np.array_equal(first[key], second[key], equal_nan=True), key
    assert np.array_equal(it_first, it_second)
    assert np.array_equal(it_first.sum(axis=1), first["iters"])
    # two shards of lp_batched_shard_bounds, solved separately and concatenated
    lib = capi.load()
    parts = []
    for shard in range(2):
        lo, hi = capi.C.c_int(), capi.C.c_int()
        assert lib.lp_batched_shard_bounds(len(cases), shard, 2, capi.C.byref(lo), capi.C.byref(hi)) == 0
        parts.append(ctx.two_phase_batched(A[lo.value:hi.value], b[lo.value:hi.value], c[lo.value:hi.value],
                                           n_orig=32))
    whole = ctx.two_phase_batched(A, b, c, n_orig=32)
    for key in ("status", "iters", "basis", "x", "obj"):
        assert np.array_equal(np.concatenate([q[key] for q in parts]), whole[key], equal_nan=True), key
    assert np.array_equal(whole["iters"], it_first)
    _assert_same(whole, _oracle(cases))


def test_fallback_handle_rerun(ctx):
    """State kept between the runs of one fallback handle: run, download, run, download."""
    cases = [lpcases.min_lp(seed, 128, 128) for seed in range(3)]
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, n_orig=128)
    try:
        assert p.path() == 0
        for g in handlecases.run_twice(p, p.phase_iters):
            _assert_same(g, _oracle(cases))
    finally:
        p.free()


@pytest.mark.parametrize("path,limit", [(1, 18), (0, 450)])
def test_handle_limit_then_rerun(ctx, path, limit):
    """A per-phase limit that stops some LPs of the batch and not others, then the default limit and the first limit
    again on the same handle; x and obj of the stopped LPs stay unwritten.  Resident: 16 x 32 + 16, phase I takes 16
    to 23 pivots; fallback: 128 x 128 + 128, phase I takes 329 to 508."""
    if path:
        cases = [lpcases.min_lp(seed, 16, 32, equalities=seed % 3, negative_rows=seed % 4) for seed in range(12)]
    else:
        cases = [lpcases.min_lp(seed, 128, 128) for seed in range(6)]
    limited, full = _oracle(cases, max_iter=limit), _oracle(cases)
    assert {r["status"] for r in limited} == {o.OPTIMAL, o.ITER_LIMIT}
    assert all(r["status"] == o.OPTIMAL for r in full)
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, n_orig=cases[0][3])
    try:
        assert p.path() == path
        first, second, third = handlecases.limit_default_limit(p, limit, p.phase_iters)
    finally:
        p.free()
    _assert_same(first, limited)
    _assert_same(second, full)
    _assert_same(third, limited)
