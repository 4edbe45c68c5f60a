"""Re-solve from a given basis (lp_simplex_resolve_run, lp_simplex_resolve, lp_simplex_resolve_batched,
lp_batched_resolve_upload / lp_batched_set_start): every LP bit for bit against tests/ref/resolve_ref.c —
status, both pivot counts and the basis; for optimal LPs also the vertex and the objective; on the single-LP
path also the pivot trace and the final tableau."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import handlecases, lpcases
from tests import resolve_ref as R

pytestmark = pytest.mark.gpu


def _cold_bases(ctx, A, b, c, basis):
    g = ctx.simplex_solve_batched(A, b, c, basis, True, A.shape[2] - A.shape[1])
    assert np.all(g["status"] == capi.OPTIMAL)
    return g["basis"]


def _refs(A, b, c, B, maximize=True, n_orig=None, max_iter=capi.MAX_ITER):
    return [R.resolve(A[k], b[k], c[k], B[k], maximize, n_orig, max_iter=max_iter) for k in range(len(A))]


def _assert_same(g, refs):
    for k, r in enumerate(refs):
        assert g["status"][k] == r["status"], (k, g["status"][k], r["status"])
        assert tuple(g["iters"][k].tolist()) == r["iters"], k
        assert np.array_equal(g["basis"][k], r["basis"]), k
        if r["status"] == capi.OPTIMAL:
            assert np.array_equal(g["x"][k], r["x"]), k   # bit for bit
            assert g["obj"][k] == r["obj"], k


def _solve(ctx, A, b, c, B, maximize=True, n_orig=None, max_iter=capi.MAX_ITER, want_path=1):
    """The handle form (checks the path), then the one-shot form; both against each other."""
    p = ctx.batched_resolve_problem(A, b, c, B, maximize=maximize, n_orig=n_orig)
    try:
        assert p.path() == want_path
        p.run(max_iter=max_iter)
        h = p.download()
        h["iters"] = p.resolve_iters()
        assert np.array_equal(h["iters"].sum(axis=1), p.download()["iters"])
    finally:
        p.free()
    g = ctx.resolve_batched(A, b, c, B, maximize=maximize, n_orig=n_orig, max_iter=max_iter)
    for key in ("status", "iters", "basis", "x", "obj"):
        assert np.array_equal(g[key], h[key], equal_nan=True), key
    return g


def _perturbed(ctx, batch, m, n, seed0):
    A, b, b2, c, basis = R.scenario(batch, m, n, seed0)
    return A, b2, c, _cold_bases(ctx, A, b, c, basis)


@pytest.mark.parametrize("m,n", [(8, 24), (32, 96), (64, 192), (100, 150), (130, 140)])
@pytest.mark.parametrize("maximize", [True, False])
def test_batched_shapes(ctx, m, n, maximize):
    A, b2, c, B = _perturbed(ctx, 40, m, n, 1000 * m)
    if not maximize:
        c = -c   # the same optimal bases
    refs = _refs(A, b2, c, B, maximize)
    g = _solve(ctx, A, b2, c, B, maximize)
    _assert_same(g, refs)
    assert sum(r["iters"][0] > 0 for r in refs) >= 20   # the dual loop ran


def _mixed_batch(ctx):
    """32 x 96 LPs of every kind: dual branch to the optimum, infeasible row, primal branch (costs changed),
    neither feasible, singular basis (repeated column), the slack basis."""
    m, n, batch = 32, 96, 36
    A, b, b2, c, basis = R.scenario(batch, m, n, 77)
    B = _cold_bases(ctx, A, b, c, basis).copy()
    rng = np.random.default_rng(5)
    for k in range(batch):
        kind = k % 6
        if kind == 1:
            b2[k, k % m] = -(1.0 + 0.1 * k) * (n - m)
        elif kind == 2:
            b2[k] = b[k]
            c[k] = c[k] * rng.uniform(0.5, 1.5, n)
        elif kind == 3:
            b2[k, k % m] = -(1.0 + 0.1 * k) * (n - m)
            nb = [j for j in range(n) if j not in set(B[k].tolist())]
            c[k, nb[k % len(nb)]] += 1e3
        elif kind == 4:
            B[k, 3] = B[k, 1]
        elif kind == 5:
            b2[k] = b[k]
            B[k] = basis[k]
    return A, b2, c, B


def test_batched_mixed_outcomes(ctx):
    A, b2, c, B = _mixed_batch(ctx)
    refs = _refs(A, b2, c, B)
    statuses = {r["status"] for r in refs}
    assert {capi.OPTIMAL, capi.INFEASIBLE, capi.BAD_ARG, capi.SINGULAR} <= statuses, statuses
    assert any(r["iters"][1] > 0 for r in refs) and any(r["iters"][0] > 0 for r in refs)
    _assert_same(_solve(ctx, A, b2, c, B), refs)
    for max_iter in (0, 1, 2, 3):
        refs = _refs(A, b2, c, B, max_iter=max_iter)
        assert any(r["status"] == capi.ITER_LIMIT for r in refs)
        _assert_same(_solve(ctx, A, b2, c, B, max_iter=max_iter), refs)


def test_batched_timing_scenario(ctx):
    """All 4096 LPs of scripts/time_resolve.py."""
    A, b2, c, B = _perturbed(ctx, 4096, 64, 192, 0)
    refs = _refs(A, b2, c, B, n_orig=128)
    g = ctx.resolve_batched(A, b2, c, B, n_orig=128)
    _assert_same(g, refs)
    assert np.all(g["status"] == capi.OPTIMAL)


def test_batched_fallback_shape(ctx):
    A, b2, c, B = _perturbed(ctx, 5, 128, 256, 31)
    refs = _refs(A, b2, c, B)
    _assert_same(_solve(ctx, A, b2, c, B, want_path=0), refs)


@pytest.mark.parametrize("path,batch,m,n,seed0,limit", [(1, 12, 32, 96, 4242, 8), (0, 6, 128, 256, 31, 20)])
def test_handle_limit_then_rerun(ctx, path, batch, m, n, seed0, limit):
    """A limit that stops some LPs of the batch and not others, then the default limit and the first limit again on
    the same handle; x and obj of the stopped LPs stay unwritten.  Resident: 0 to 22 dual pivots; fallback: 1 to 56."""
    A, b2, c, B = _perturbed(ctx, batch, m, n, seed0)
    limited, full = _refs(A, b2, c, B, max_iter=limit), _refs(A, b2, c, B)
    assert {r["status"] for r in limited} == {capi.OPTIMAL, capi.ITER_LIMIT}
    assert all(r["status"] == capi.OPTIMAL for r in full)
    p = ctx.batched_resolve_problem(A, b2, c, B)
    try:
        assert p.path() == path
        first, second, third = handlecases.limit_default_limit(p, limit, p.resolve_iters)
    finally:
        p.free()
    _assert_same(first, limited)
    _assert_same(second, full)
    _assert_same(third, limited)


@pytest.mark.parametrize("m,n", [(32, 96), (128, 256)])
def test_handle_set_start_twice(ctx, m, n):
    """The branch-and-bound loop: run, download the bases, change b, set_start, run again."""
    A, b2, c, B = _perturbed(ctx, 6, m, n, 4242)
    p = ctx.batched_resolve_problem(A, b2, c, B)
    try:
        b_now, B_now = b2, B
        for step in range(3):
            p.run()
            h = p.download()
            h["iters"] = p.resolve_iters()
            _assert_same(h, _refs(A, b_now, c, B_now))
            g = ctx.resolve_batched(A, b_now, c, B_now)
            for key in ("status", "iters", "basis", "x", "obj"):
                assert np.array_equal(g[key], h[key], equal_nan=True), (step, key)
            b_now = np.stack([R.scale_rows(500 + 10 * step + k, b_now[k], 0.8, 0.95) for k in range(len(A))])
            B_now = h["basis"]
            p.set_start(b=b_now, basis=B_now)
        bad = B_now.copy()
        bad[0, 0] = n
        with pytest.raises(capi.LPError):
            p.set_start(basis=bad)
        with pytest.raises(capi.LPError):
            p.phase_iters()
    finally:
        p.free()


def test_other_batch_kinds_refuse_resolve_calls(ctx):
    A, b, b2, c, basis = R.scenario(4, 8, 24)
    for q in (ctx.batched_problem(A, b, c, basis), ctx.batched_two_phase_problem(A, b, c, maximize=True)):
        try:
            with pytest.raises(capi.LPError):
                q.set_start(b=b2)
            with pytest.raises(capi.LPError):
                q.resolve_iters()
        finally:
            q.free()
    p = ctx.batched_resolve_problem(A, b2, c, basis)
    p.set_pivot_rule("bland")
    with pytest.raises(capi.LPError):
        p.run()
    p.free()


def _single_case(ctx, seed, m, n, cost_change=False):
    A, b, c, basis = lpcases.random_lp(seed, m, n)
    cold = ctx.simplex_solve(A, b, c, basis, True, n - m)
    assert cold["status"] == capi.OPTIMAL
    if cost_change:
        c = c * np.random.default_rng(seed).uniform(0.5, 1.5, n)
    else:
        b = R.scale_rows(seed, b)
    return A, b, c, cold["basis"]


@pytest.mark.parametrize("seed,m,n,cost_change,algo", [
    (0, 512, 1024, False, capi.SIMPLEX_LAUNCH),
    (1, 1024, 1200, False, capi.SIMPLEX_LAUNCH),
    (2, 512, 1024, True, capi.SIMPLEX_RESIDENT),
])
def test_single_lp(ctx, seed, m, n, cost_change, algo):
    A, b, c, B = _single_case(ctx, seed, m, n, cost_change)
    r = R.resolve(A, b, c, B, True, n - m, trace_cap=1 << 14, want_tableau=True)
    assert r["status"] == capi.OPTIMAL
    assert (r["iters"][1] if cost_change else r["iters"][0]) > 0
    p = ctx.simplex_problem(A, b, c, B, True, n - m)
    try:
        for _ in range(2):   # (lp_simplex_reset restores the crashed tableau: the run repeats)
            p.reset()
            rc, st, iters = p.resolve()
            assert (rc, iters, st.algo_used, st.fell_back) == (r["status"], r["iters"], algo, 0)
            g = p.download(trace_cap=sum(iters), want_tableau=True)
            assert list(zip(g["trace_enter"].tolist(), g["trace_leave"].tolist())) == r["trace"]
            assert np.array_equal(g["basis"], r["basis"])
            assert np.array_equal(g["x"], r["x"]) and g["obj"] == r["obj"]
            assert np.array_equal(g["tableau"], r["tableau"])
    finally:
        p.free()
    o = ctx.simplex_resolve(A, b, c, B, True, n - m)
    assert (o["status"], o["iters"], o["obj"]) == (r["status"], r["iters"], r["obj"])
    assert np.array_equal(o["x"], r["x"]) and np.array_equal(o["basis"], r["basis"])


def test_single_lp_outcomes(ctx):
    """Infeasible, neither feasible (LP_BAD_ARG), singular and the iteration limit on the one-shot call."""
    A, b, c, B = _single_case(ctx, 9, 48, 120)
    no = 72
    b_inf = b.copy()
    b_inf[5] = -50.0   # (every coefficient of a gen_lp row is >= 0)
    r = R.resolve(A, b_inf, c, B, True, no)
    g = ctx.simplex_resolve(A, b_inf, c, B, True, no)
    assert g["status"] == r["status"] == capi.INFEASIBLE and g["iters"] == r["iters"]
    assert np.array_equal(g["basis"], r["basis"])
    c_bad = c.copy()
    c_bad[[j for j in range(120) if j not in set(B.tolist())][0]] += 1e3
    assert R.resolve(A, b_inf, c_bad, B, True, no)["status"] == capi.BAD_ARG
    with pytest.raises(capi.LPError) as e:
        ctx.simplex_resolve(A, b_inf, c_bad, B, True, no)
    assert e.value.code == capi.BAD_ARG
    Bs = B.copy()
    Bs[2] = Bs[0]
    assert ctx.simplex_resolve(A, b, c, Bs, True, no)["status"] == capi.SINGULAR == R.resolve(A, b, c, Bs)["status"]
    for max_iter in (1, 2):
        r = R.resolve(A, b, c, B, True, no, max_iter=max_iter)
        g = ctx.simplex_resolve(A, b, c, B, True, no, max_iter=max_iter)
        assert g["status"] == r["status"] == capi.ITER_LIMIT and g["iters"] == r["iters"]
        assert np.array_equal(g["basis"], r["basis"])
    p = ctx.simplex_problem(A, b, c, B, True, no)
    p.set_pivot_rule("bland")
    with pytest.raises(capi.LPError):
        p.resolve()
    p.free()
