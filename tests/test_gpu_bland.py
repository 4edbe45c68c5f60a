"""GPU: Bland's pivot rule (LP_PIVOT_BLAND) on the launch path, the single-LP two-phase flow and both
batched kernels, every result bit-exact against the test restatement tests/ref/bland_ref.c."""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import bland_ref as R
from tests import lpcases

pytestmark = pytest.mark.gpu

BEALE_TRACE = [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (0, 1), (2, 2)]
CYCLING = [(64, 128, 7), (256, 512, 7), (1024, 2048, 8)]


def _run(ctx, A, b, c, basis, maximize, n_orig, algo=capi.SIMPLEX_AUTO, rule="bland", max_iter=capi.MAX_ITER):
    p = ctx.simplex_problem(A, b, c, basis, maximize, n_orig)
    try:
        p.set_pivot_rule(rule)
        rc, st = p.run(max_iter=max_iter, algo=algo)
        out = p.download(trace_cap=max(st.pivots, 1), want_tableau=True)
    finally:
        p.free()
    out.update(status=rc, iters=st.pivots, algo_used=st.algo_used, fell_back=st.fell_back)
    return out


def _assert_bit_exact(g, r):
    assert g["status"] == r["status"]
    assert g["iters"] == r["iters"]
    k = r["iters"]
    assert list(zip(g["trace_enter"][:k].tolist(), g["trace_leave"][:k].tolist())) == r["trace"][:k]
    assert np.array_equal(g["basis"], r["basis"])
    if r["status"] == o.OPTIMAL:
        assert np.array_equal(g["x"], r["x"]) and g["obj"] == r["obj"]
    assert np.array_equal(g["tableau"], r["tableau"])


def _ref(A, b, c, basis, maximize, no, rule=R.BLAND, max_iter=capi.MAX_ITER):
    return R.simplex_tableau(A, b, c, basis, maximize, no, rule=rule, max_iter=max_iter, trace_cap=1 << 14,
                             want_tableau=True)


# ---- single LP, launch pair

@pytest.mark.parametrize("algo", [capi.SIMPLEX_AUTO, capi.SIMPLEX_LAUNCH])
def test_beale_single(ctx, algo):
    A, b, c, basis, no = R.beale()
    g = _run(ctx, A, b, c, basis, True, no, algo=algo)
    assert g["status"] == capi.OPTIMAL and g["iters"] == 7 and g["algo_used"] == capi.SIMPLEX_LAUNCH
    assert list(zip(g["trace_enter"].tolist(), g["trace_leave"].tolist())) == BEALE_TRACE
    assert g["obj"] == 1.0 and g["x"].tolist() == [1.0, 0.0, 1.0, 0.0]
    _assert_bit_exact(g, _ref(A, b, c, basis, True, no))
    r = ctx.simplex_solve(A, b, c, basis, True, no, pivot_rule="bland")
    assert r["status"] == capi.OPTIMAL and r["iters"] == 7 and r["obj"] == 1.0
    d = ctx.simplex_solve(A, b, c, basis, True, no)   # the default rule still cycles
    assert d["status"] == capi.ITER_LIMIT and d["iters"] == capi.MAX_ITER


@pytest.mark.parametrize("m,n,seed", CYCLING)
def test_cycling_family_single(ctx, m, n, seed):
    A, b, c, basis, no = R.cycling_lp(seed, m, n)
    assert R.simplex_tableau(A, b, c, basis, True, no, rule=R.DANTZIG)["status"] == o.ITER_LIMIT
    r = _ref(A, b, c, basis, True, no)
    assert r["status"] == o.OPTIMAL
    g = _run(ctx, A, b, c, basis, True, no)
    assert g["algo_used"] == capi.SIMPLEX_LAUNCH
    _assert_bit_exact(g, r)


@pytest.mark.parametrize("seed,m,n", [(0, 2, 5), (1, 8, 16), (2, 16, 32), (3, 33, 71), (4, 64, 128),
                                       (5, 128, 256), (6, 100, 1500)])
def test_random_lp_single(ctx, seed, m, n):
    A, b, c, basis = lpcases.random_lp(seed, m, n)
    r = _ref(A, b, c, basis, True, n - m)
    assert r["status"] == o.OPTIMAL and r["iters"] > 0
    _assert_bit_exact(_run(ctx, A, b, c, basis, True, n - m, algo=capi.SIMPLEX_LAUNCH), r)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_general_basis_single(ctx, seed):
    """Non-slack starting basis (the crash runs first), minimisation and maximisation."""
    A, b, c, basis = lpcases.general_lp(seed, 12, 30)
    for mx in (True, False):
        _assert_bit_exact(_run(ctx, A, b, c, basis, mx, A.shape[1]), _ref(A, b, c, basis, mx, A.shape[1]))


def test_rule_switch_leaves_no_state(ctx):
    A, b, c, basis = lpcases.random_lp(5, 128, 256)
    no = 128
    p = ctx.simplex_problem(A, b, c, basis, True, no)
    try:
        p.set_pivot_rule("bland")
        rc, st = p.run()
        gb = p.download(trace_cap=st.pivots, want_tableau=True)
        gb.update(status=rc, iters=st.pivots)
        _assert_bit_exact(gb, _ref(A, b, c, basis, True, no))
        p.reset()
        p.set_pivot_rule("dantzig")
        rc, st = p.run(algo=capi.SIMPLEX_LAUNCH)
        gd = p.download(trace_cap=st.pivots, want_tableau=True)
        gd.update(status=rc, iters=st.pivots)
    finally:
        p.free()
    q = o.simplex_tableau(A, b, c, basis, True, no, trace_cap=1 << 14, want_tableau=True)
    _assert_bit_exact(gd, q)
    assert gb["iters"] != gd["iters"] or gb["trace_enter"].tolist() != gd["trace_enter"].tolist()


@pytest.mark.parametrize("algo", [capi.SIMPLEX_RESIDENT, capi.SIMPLEX_LOOKAHEAD, capi.SIMPLEX_OVERLAP])
def test_other_algorithms_refuse_bland(ctx, algo):
    A, b, c, basis = lpcases.random_lp(4, 64, 128)
    p = ctx.simplex_problem(A, b, c, basis, True, 64)
    try:
        p.set_pivot_rule("bland")
        with pytest.raises(capi.LPError) as e:
            p.run(algo=algo)
        assert e.value.code == capi.BAD_ARG and "Bland" in ctx.error()
        with pytest.raises(capi.LPError):
            p.set_pivot_rule(5)
    finally:
        p.free()


# ---- single-LP two-phase

def _two_phase_cases():
    cases = [lpcases.min_lp(s, m, k, equalities=e, negative_rows=nr, zero_rhs=z)
             for s, (m, k, e, nr, z) in enumerate([(5, 4, 0, 0, 0), (8, 6, 1, 2, 1), (12, 10, 2, 0, 2),
                                                   (16, 24, 0, 3, 0), (32, 40, 3, 2, 2)])]
    cases += [lpcases.degenerate_eq_lp(s) for s in (0, 1, 2)]
    for g in json.load(open(os.path.join(os.path.dirname(__file__), "golden", "two_phase_cases.json"))):
        if g["kind"] == "min":
            a = g["args"]
            cases.append(lpcases.min_lp(g["seed"], a[0], a[1], equalities=a[2], negative_rows=a[3], zero_rhs=a[4]))
        else:
            cases.append(lpcases.degenerate_eq_lp(g["seed"]))
    return cases


def _assert_two_phase(g, r):
    assert g["status"] == r["status"] and list(g["iters"]) == list(r["iters"])
    assert np.array_equal(g["basis"], r["basis"])
    if r["status"] == o.OPTIMAL:
        assert np.array_equal(g["x"], r["x"]) and g["obj"] == r["obj"]


def test_two_phase_beale(ctx):
    A, b, c, _, no = R.beale()
    for mx, cost in ((True, c), (False, -c)):
        r = R.two_phase(A, b, cost, mx, no, rule=R.BLAND)
        assert r["status"] == o.OPTIMAL
        _assert_two_phase(ctx.two_phase(A, b, cost, mx, no, pivot_rule="bland"), r)
        assert ctx.two_phase(A, b, cost, mx, no)["status"] == capi.ITER_LIMIT


def test_two_phase_mixes(ctx):
    for A, b, c, no in _two_phase_cases():
        for mx in (False, True):
            _assert_two_phase(ctx.two_phase(A, b, c, mx, no, pivot_rule="bland"),
                              R.two_phase(A, b, c, mx, no, rule=R.BLAND))


# ---- batched plain

def _stack(cases):
    return (np.stack([q[0] for q in cases]), np.stack([q[1] for q in cases]), np.stack([q[2] for q in cases]),
            np.stack([q[3] for q in cases]))


def _assert_batched(g, refs):
    for k, r in enumerate(refs):
        assert g["status"][k] == r["status"], k
        assert g["iters"][k] == r["iters"], k
        assert np.array_equal(g["basis"][k], r["basis"]), k
        if r["status"] == o.OPTIMAL:
            assert np.array_equal(g["x"][k], r["x"]), k
            assert g["obj"][k] == r["obj"], k


def _batch_refs(cases, no, max_iter=capi.MAX_ITER):
    return [R.simplex_tableau(A, b, c, basis, True, no, rule=R.BLAND, max_iter=max_iter) for A, b, c, basis in cases]


def test_batched_4096_with_cycling(ctx):
    m, n = 128, 256
    cases = []
    for k in range(4096):
        if k % 8 == 3:
            A, b, c, basis, _ = R.cycling_lp(k, m, n, blocks=1 + k % 3)
        else:
            A, b, c, basis = lpcases.random_lp(k, m, n)
        cases.append((A, b, c, basis))
    for k in (3, 11):
        assert R.simplex_tableau(*cases[k], True, m, rule=R.DANTZIG)["status"] == o.ITER_LIMIT
    refs = _batch_refs(cases, m)
    A, b, c, basis = _stack(cases)
    p = ctx.batched_problem(A, b, c, basis, True, m)
    try:
        assert p.path() == 1
        p.set_pivot_rule("bland")
        p.run()
        _assert_batched(p.download(), refs)
    finally:
        p.free()


def test_batched_mixed_outcomes(ctx):
    m, n = 64, 128
    cases = [R.cycling_lp(s, m, n)[:4] if s % 4 == 0 else lpcases.random_lp(s, m, n) for s in range(64)]
    cases[5] = (cases[5][0] * np.where(np.arange(n) < m, -1.0, 1.0), cases[5][1], cases[5][2], cases[5][3])  # unbounded
    refs = _batch_refs(cases, m, max_iter=150)
    assert {r["status"] for r in refs} >= {o.OPTIMAL, o.ITER_LIMIT, o.UNBOUNDED}
    A, b, c, basis = _stack(cases)
    _assert_batched(ctx.simplex_solve_batched(A, b, c, basis, True, m, max_iter=150, pivot_rule="bland"), refs)


def test_batched_fallback_shape(ctx):
    """A non-identity starting basis takes the per-LP fallback, which carries the rule."""
    cases = [lpcases.general_lp(s, 10, 24) for s in range(6)]
    A, b, c, basis = _stack(cases)
    no = A.shape[2]
    refs = [R.simplex_tableau(*q, True, no, rule=R.BLAND) for q in cases]
    p = ctx.batched_problem(A, b, c, basis, True, no)
    try:
        assert p.path() == 0
        p.set_pivot_rule("bland")
        p.run()
        _assert_batched(p.download(), refs)
    finally:
        p.free()


# ---- batched two-phase

def _tp_stack(cases):
    return np.stack([q[0] for q in cases]), np.stack([q[1] for q in cases]), np.stack([q[2] for q in cases])


def _assert_tp_batched(g, refs):
    for k, r in enumerate(refs):
        assert g["status"][k] == r["status"], k
        assert g["iters"][k].tolist() == list(r["iters"]), k
        assert np.array_equal(g["basis"][k], r["basis"]), k
        if r["status"] == o.OPTIMAL:
            assert np.array_equal(g["x"][k], r["x"]), k
            assert g["obj"][k] == r["obj"], k


@pytest.mark.parametrize("m,k", [(2, 3), (5, 4), (8, 16), (16, 32), (32, 64), (64, 128)])
def test_batched_two_phase_shapes(ctx, m, k):
    cases = [lpcases.min_lp(s, m, k, equalities=s % min(m, 3), negative_rows=s % 2, zero_rhs=s % 2)
             for s in range(96)]
    refs = [R.two_phase(A, b, c, False, no, rule=R.BLAND) for A, b, c, no in cases]
    A, b, c = _tp_stack(cases)
    _assert_tp_batched(ctx.two_phase_batched(A, b, c, False, k, pivot_rule="bland"), refs)


def test_batched_two_phase_cycling(ctx):
    A1, b1, c1, _, no = R.beale()
    cases = []
    for s in range(32):
        if s % 2 == 0:
            cases.append((A1, b1, c1 * (1.0 + s), no))
        else:
            cases.append((A1, b1, -c1, no))
    refs = [R.two_phase(A, b, c, s % 2 == 0, no, rule=R.BLAND) for s, (A, b, c, no) in enumerate(cases)]
    assert all(r["status"] == o.OPTIMAL for r in refs)
    for mx in (True, False):
        sel = [s for s in range(32) if (s % 2 == 0) == mx]
        A, b, c = _tp_stack([cases[s] for s in sel])
        _assert_tp_batched(ctx.two_phase_batched(A, b, c, mx, no, pivot_rule="bland"), [refs[s] for s in sel])


def test_batched_two_phase_fallback_and_handle(ctx):
    m, k = 128, 128   # (m+1) x (m+k+1) doubles: beyond one CU's LDS
    cases = [lpcases.min_lp(s, m, k) for s in range(3)]
    refs = [R.two_phase(A, b, c, False, no, rule=R.BLAND) for A, b, c, no in cases]
    A, b, c = _tp_stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, False, k)
    try:
        assert p.path() == 0
        p.set_pivot_rule("bland")
        p.run()
        g = p.download()
        g["iters"] = p.phase_iters()
        _assert_tp_batched(g, refs)
    finally:
        p.free()
    cases = [lpcases.min_lp(s, 16, 24, zero_rhs=1) for s in range(48)]
    refs = [R.two_phase(A, b, c, False, no, rule=R.BLAND) for A, b, c, no in cases]
    A, b, c = _tp_stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, False, 24)
    try:
        assert p.path() == 1
        p.set_pivot_rule("bland")
        for _ in range(2):   # the handle runs again with the same answer
            p.run()
            g = p.download()
            g["iters"] = p.phase_iters()
            _assert_tp_batched(g, refs)
    finally:
        p.free()
