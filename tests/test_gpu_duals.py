"""The dual solution at a basis on the GPU (lp_basis_duals, lp_basis_duals_batched, lp_batched_duals): y, d, w
and the status bit for bit against tests/ref/duals_ref.c on both sides of lp_basis_duals_fits, after plain,
two-phase and re-solve batch runs and on the per-LP fallback; beyond that, strong duality against the solve's
own objective and the same duals at the enumeration's winning basis."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import certcases as CC
from tests import duals_ref as D
from tests import lpcases
from tests import resolve_ref as R

pytestmark = pytest.mark.gpu


def _same(g, r):
    """Bit for bit, NaN where the reference has NaN."""
    assert np.array_equal(np.asarray(g["status"]), np.asarray(r["status"]))
    for key in ("y", "d", "w"):
        a, b = np.atleast_1d(np.asarray(g[key], dtype=np.float64)), np.atleast_1d(np.asarray(r[key], dtype=np.float64))
        nan = np.isnan(a)
        assert np.array_equal(nan, np.isnan(b)), key
        assert np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)), key   # signed zeros included


def _strong(w, z):
    assert abs(w - z) <= 1e-9 * (1 + abs(z)), (w, z)


def _stack(cases):
    return (np.stack([k[0] for k in cases]), np.stack([k[1] for k in cases]), np.stack([k[2] for k in cases]))


@pytest.mark.parametrize("m,n", [(128, 256), (512, 1024)])
@pytest.mark.parametrize("maximize", [True, False])
def test_single_lp_both_sides_of_fits(ctx, m, n, maximize):
    assert ctx.basis_duals_fits(m) == (m <= 140)
    A, b, c, basis = capi.gen_lp(7 * m + int(maximize), m, n)
    if not maximize:
        c = -c   # min -c.x: the optimum of the max problem, reduced costs of the other sign
    s = ctx.simplex_solve(A, b, c, basis, maximize, n)
    assert s["status"] == capi.OPTIMAL
    g = ctx.basis_duals(A, b, c, s["basis"])
    r = D.duals(A, b, c, s["basis"])
    _same(g, r)
    assert g["status"] == capi.OPTIMAL
    _strong(g["w"], s["obj"])
    assert (g["d"].max() <= 1e-9) if maximize else (g["d"].min() >= -1e-9)
    assert np.array_equal(g["d"][s["basis"]], np.zeros(m))
    # the batched call with one LP: the same bits
    h = ctx.basis_duals_batched(A[None], b[None], c[None], s["basis"][None])
    assert h["status"][0] == g["status"]
    for key in ("y", "d"):
        assert np.array_equal(h[key][0], g[key])
    assert h["w"][0] == g["w"]


def test_plain_batch_4096(ctx):
    batch, m, n = 4096, 128, 256
    cases = [capi.gen_lp(seed, m, n) for seed in range(batch)]
    A, b, c = _stack(cases)
    basis = np.stack([k[3] for k in cases])
    p = ctx.batched_problem(A, b, c, basis, True, n - m)
    try:
        assert p.path() == 1
        with pytest.raises(capi.LPError) as e:
            p.duals()   # before the first run
        assert e.value.code == capi.BAD_ARG
        p.run()
        s = p.download()
        g = p.duals()
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, D.duals_batched(A, b, c, s["basis"], s["status"]))
    for k in range(0, batch, 97):
        _strong(g["w"][k], s["obj"][k])


def test_two_phase_batch_4096(ctx):
    batch, m, k = 4096, 64, 128
    cases = [lpcases.min_lp(seed, m, k) for seed in range(batch)]
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=m + k)
    try:
        assert p.path() == 1
        p.run()
        s = p.download()
        g = p.duals()
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, D.duals_batched(A, b, c, s["basis"], s["status"]))
    for j in range(0, batch, 97):
        _strong(g["w"][j], s["obj"][j])
        assert g["d"][j].min() >= -1e-9


def test_resolve_batch(ctx):
    batch, m, n = 256, 32, 96
    A, b, b2, c, basis = R.scenario(batch, m, n, 500)
    cold = ctx.simplex_solve_batched(A, b, c, basis, True, n - m)
    assert (cold["status"] == capi.OPTIMAL).all()
    p = ctx.batched_resolve_problem(A, b2, c, cold["basis"], True, n)
    try:
        assert p.path() == 1
        p.run()
        s = p.download()
        g = p.duals()
        p.set_start(b=b)   # back to the old right-hand sides: the duals follow the new run
        p.run()
        s2 = p.download()
        g2 = p.duals()
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, D.duals_batched(A, b2, c, s["basis"], s["status"]))
    _same(g2, D.duals_batched(A, b, c, s2["basis"], s2["status"]))
    for k in range(batch):
        _strong(g["w"][k], s["obj"][k])


def test_fallback_handle(ctx):
    cases = [lpcases.min_lp(seed, 128, 128) for seed in range(3)]
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=256)
    try:
        assert p.path() == 0
        p.run()
        s = p.download()
        g = p.duals()
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, D.duals_batched(A, b, c, s["basis"], s["status"]))
    for k in range(3):
        _strong(g["w"][k], s["obj"][k])


def test_fallback_handle_keeps_run_statuses(ctx):
    """A plain fallback handle with unbounded LPs (test_gpu_certificate's): only the LP_OPTIMAL ones get duals."""
    A, b, c, basis, names = CC.plain_mix(40, 6, 16, 40)
    basis = basis[:, ::-1].copy()   # the slack basis, positions reversed
    p = ctx.batched_problem(A, b, c, basis, True)
    try:
        assert p.path() == 0
        p.run()
        s = p.download()
        g = p.duals()
    finally:
        p.free()
    assert [int(v) for v in s["status"]] == [0 if f == "optimal" else 1 for f in names]
    _same(g, D.duals_batched(A, b, c, s["basis"], s["status"]))


def test_mixed_batch_keeps_run_statuses(ctx):
    m, k = 16, 32
    cases = []
    for seed in range(24):
        A, b, c, _ = lpcases.min_lp(seed, m, k)
        A, c = A.copy(), c.copy()
        if seed % 4 == 1:   # A0_i x - s_i = b_i with A0_i <= 0 and b_i > 0: infeasible
            A[3, :k] = -A[3, :k]
        elif seed % 4 == 2:   # a negative cost on a column that only helps A0 x >= b: unbounded
            c[5] = -1.0
        cases.append((A, b, c))
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=m + k)
    try:
        assert p.path() == 1
        p.run()
        s = p.download()
        g = p.duals()
    finally:
        p.free()
    want = np.array([[capi.OPTIMAL, capi.INFEASIBLE, capi.UNBOUNDED, capi.OPTIMAL][seed % 4] for seed in range(24)])
    assert np.array_equal(s["status"], want)
    assert np.array_equal(g["status"], want)
    bad = want != capi.OPTIMAL
    assert np.isnan(g["y"][bad]).all() and np.isnan(g["d"][bad]).all() and np.isnan(g["w"][bad]).all()
    _same(g, D.duals_batched(A, b, c, s["basis"], s["status"]))


@pytest.mark.parametrize("m,n", [(24, 60), (200, 400)])
def test_singular_and_out_of_range(ctx, m, n):
    A, b, c, basis = capi.gen_lp(11, m, n)
    Bs = basis.copy()
    Bs[3] = Bs[1]   # repeated index
    g = ctx.basis_duals(A, b, c, Bs)
    assert g["status"] == capi.SINGULAR
    _same(g, D.duals(A, b, c, Bs))
    Bo = basis.copy()
    Bo[2] = n
    with pytest.raises(capi.LPError) as e:
        ctx.basis_duals(A, b, c, Bo)
    assert e.value.code == capi.BAD_ARG
    # batched: the statuses are per LP
    s = ctx.simplex_solve(A, b, c, basis, True, n - m)
    bases = np.stack([s["basis"], Bs, Bo, basis])
    Ab, bb, cb = np.stack([A] * 4), np.stack([b] * 4), np.stack([c] * 4)
    h = ctx.basis_duals_batched(Ab, bb, cb, bases)
    assert h["status"].tolist() == [capi.OPTIMAL, capi.SINGULAR, capi.BAD_ARG, capi.OPTIMAL]
    assert np.isnan(h["y"][2]).all() and np.isnan(h["d"][2]).all() and np.isnan(h["w"][2])
    _same(h, D.duals_batched(Ab, bb, cb, bases))
    assert np.array_equal(h["y"][3], c[basis])   # the slack identity: y = c_B


def test_enumeration_basis_gives_the_same_duals(ctx):
    checked = 0
    for seed in range(12):
        m, n = 5 + seed % 3, 12 + seed % 4
        A, b, c, basis = capi.gen_lp(100 + seed, m, n)
        e = ctx.enum_solve(A, b, c, True, n)
        s = ctx.simplex_solve(A, b, c, basis, True, n)
        assert e["status"] == s["status"] == capi.OPTIMAL
        if sorted(e["basis"].tolist()) != sorted(s["basis"].tolist()):
            continue   # (a degenerate or tied optimum: not unique)
        ge = ctx.basis_duals(A, b, c, e["basis"])
        gs = ctx.basis_duals(A, b, c, s["basis"])
        _same(ge, D.duals(A, b, c, e["basis"]))
        assert np.allclose(ge["y"], gs["y"], rtol=1e-12, atol=1e-12)
        assert np.allclose(ge["d"], gs["d"], rtol=1e-12, atol=1e-12)
        _strong(ge["w"], e["obj"])
        checked += 1
    assert checked >= 8
