"""RHS and cost ranging at a basis on the GPU (lp_basis_ranging, lp_basis_ranging_batched, lp_batched_ranging): every
end, every leaving / entering index and the status bit for bit against tests/ref/ranging_ref.c on both sides of
lp_basis_ranging_fits, after plain, two-phase and re-solve batch runs and on the per-LP fallback."""
import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import certcases as CC
from tests import duals_ref as D
from tests import lpcases
from tests import ranging_ref as RR
from tests import resolve_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("b_lo", "b_hi", "c_lo", "c_hi")


def _same(g, r):
    """Bit for bit, NaN where the reference has NaN, indices equal."""
    assert np.array_equal(np.asarray(g["status"]), np.asarray(r["status"]))
    for key in KEYS:
        a, b = np.asarray(g[key], dtype=np.float64), np.asarray(r[key], dtype=np.float64)
        nan = np.isnan(a)
        assert np.array_equal(nan, np.isnan(b)), key
        assert np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)), key   # signed zeros included
    assert np.array_equal(g["b_leave"], r["b_leave"])
    assert np.array_equal(g["c_enter"], r["c_enter"])


def _stack(cases):
    return (np.stack([k[0] for k in cases]), np.stack([k[1] for k in cases]), np.stack([k[2] for k in cases]))


@pytest.mark.parametrize("m,n", [(96, 200), (128, 256), (512, 1024)])
@pytest.mark.parametrize("maximize", [True, False])
def test_single_lp_both_sides_of_fits(ctx, m, n, maximize):
    assert ctx.basis_ranging_fits(m, n) == (m <= 128)
    A, b, c, basis = capi.gen_lp(5 * m + int(maximize), m, n)
    if not maximize:
        c = -c   # min -c.x: the optimum of the max problem, the cost sides swapped
    s = ctx.simplex_solve(A, b, c, basis, maximize, n)
    assert s["status"] == capi.OPTIMAL
    g = ctx.basis_ranging(A, b, c, s["basis"], maximize)
    _same(g, RR.ranging(A, b, c, s["basis"], maximize))
    assert g["status"] == capi.OPTIMAL
    assert (g["b_lo"] <= b + 1e-9).all() and (b <= g["b_hi"] + 1e-9).all()
    assert (g["c_lo"] <= c + 1e-9).all() and (c <= g["c_hi"] + 1e-9).all()
    h = ctx.basis_ranging_batched(A[None], b[None], c[None], s["basis"][None], maximize)   # batch of one
    assert h["status"][0] == g["status"]
    for key in KEYS + ("b_leave", "c_enter"):
        assert np.array_equal(h[key][0], g[key])


def test_plain_batch_4096(ctx):
    batch, m, n = 4096, 128, 256
    cases = [capi.gen_lp(seed, m, n) for seed in range(batch)]
    A, b, c = _stack(cases)
    basis = np.stack([k[3] for k in cases])
    p = ctx.batched_problem(A, b, c, basis, True, n - m)
    try:
        assert p.path() == 1
        with pytest.raises(capi.LPError) as e:
            p.ranging()   # before the first run
        assert e.value.code == capi.BAD_ARG
        p.run()
        s = p.download()
        g = p.ranging()
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, RR.ranging_batched(A, b, c, s["basis"], True, run_status=s["status"]))


def test_two_phase_batch_4096(ctx):
    batch, m, k = 4096, 64, 128
    cases = [lpcases.min_lp(seed, m, k) for seed in range(batch)]
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=m + k)
    try:
        assert p.path() == 1
        p.run()
        s = p.download()
        g = p.ranging()
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, RR.ranging_batched(A, b, c, s["basis"], False, run_status=s["status"]))


def test_two_phase_sign_flipped_rows_do_not_show(ctx):
    cases = [lpcases.min_lp(seed, 12, 20, negative_rows=4) for seed in range(64)]
    A, b, c = _stack(cases)
    assert (b[:, :4] < 0).all()
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=32)
    try:
        p.run()
        s = p.download()
        g = p.ranging()
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, RR.ranging_batched(A, b, c, s["basis"], False, run_status=s["status"]))
    assert (g["b_lo"] <= b + 1e-9).all() and (b <= g["b_hi"] + 1e-9).all()   # around the caller's b


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
        g = p.ranging()
        g0 = p.ranging(eps=0.0)
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, RR.ranging_batched(A, b2, c, s["basis"], True, run_status=s["status"]))
    _same(g0, RR.ranging_batched(A, b2, c, s["basis"], True, eps=0.0, run_status=s["status"]))


def test_fallback_handle(ctx):
    cases = [lpcases.min_lp(seed, 136, 136) for seed in range(2)]   # beyond lp_basis_ranging_fits as well
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=272)
    try:
        assert p.path() == 0
        p.run()
        s = p.download()
        g = p.ranging()
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, RR.ranging_batched(A, b, c, s["basis"], False, run_status=s["status"]))


def test_fallback_handle_keeps_run_statuses(ctx):
    """A plain fallback handle with unbounded LPs (test_gpu_certificate's): only the LP_OPTIMAL ones get ranges."""
    A, b, c, basis, names = CC.plain_mix(40, 6, 16, 40)
    basis = basis[:, ::-1].copy()   # the slack basis, positions reversed
    p = ctx.batched_problem(A, b, c, basis, True)
    try:
        assert p.path() == 0
        p.run()
        s = p.download()
        g = p.ranging()
    finally:
        p.free()
    assert [int(v) for v in s["status"]] == [0 if f == "optimal" else 1 for f in names]
    _same(g, RR.ranging_batched(A, b, c, s["basis"], True, run_status=s["status"]))


def test_mixed_batch_keeps_run_statuses(ctx):
    m, k = 16, 32
    cases = []
    for seed in range(24):
        A, b, c, _ = lpcases.min_lp(seed, m, k)
        A, c = A.copy(), c.copy()
        if seed % 4 == 1:   # infeasible
            A[3, :k] = -A[3, :k]
        elif seed % 4 == 2:   # unbounded
            c[5] = -1.0
        cases.append((A, b, c))
    A, b, c = _stack(cases)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=m + k)
    try:
        p.run()
        s = p.download()
        g = p.ranging()
    finally:
        p.free()
    want = np.array([[capi.OPTIMAL, capi.INFEASIBLE, capi.UNBOUNDED, capi.OPTIMAL][seed % 4] for seed in range(24)])
    assert np.array_equal(s["status"], want) and np.array_equal(g["status"], want)
    bad = want != capi.OPTIMAL
    assert np.isnan(g["b_lo"][bad]).all() and np.isnan(g["c_hi"][bad]).all() and (g["c_enter"][bad] == -1).all()
    _same(g, RR.ranging_batched(A, b, c, s["basis"], False, run_status=s["status"]))


@pytest.mark.parametrize("m,n", [(24, 60), (200, 400)])
def test_singular_and_out_of_range(ctx, m, n):
    A, b, c, basis = capi.gen_lp(11, m, n)
    Bs = basis.copy()
    Bs[3] = Bs[1]   # repeated index
    g = ctx.basis_ranging(A, b, c, Bs)
    assert g["status"] == capi.SINGULAR
    _same(g, RR.ranging(A, b, c, Bs))
    Bo = basis.copy()
    Bo[2] = n
    with pytest.raises(capi.LPError) as e:
        ctx.basis_ranging(A, b, c, Bo)
    assert e.value.code == capi.BAD_ARG
    with pytest.raises(capi.LPError) as e:
        ctx.basis_ranging(A, b, c, basis, eps=-1.0)
    assert e.value.code == capi.BAD_ARG
    s = ctx.simplex_solve(A, b, c, basis, True, n - m)
    bases = np.stack([s["basis"], Bs, Bo, basis])
    Ab, bb, cb = np.stack([A] * 4), np.stack([b] * 4), np.stack([c] * 4)
    h = ctx.basis_ranging_batched(Ab, bb, cb, bases)
    assert h["status"].tolist() == [capi.OPTIMAL, capi.SINGULAR, capi.BAD_ARG, capi.OPTIMAL]
    assert np.isnan(h["b_lo"][2]).all() and (h["b_leave"][2] == -1).all()
    _same(h, RR.ranging_batched(Ab, bb, cb, bases))


@pytest.mark.parametrize("seed", range(6))
def test_degenerate_lp_ties_and_signed_zeros(ctx, seed):
    A, b, c, k = lpcases.degenerate_eq_lp(seed)
    q = o.two_phase(A, b, c, False, A.shape[1])
    assert q["status"] == o.OPTIMAL
    r = RR.ranging(A, b, c, q["basis"], False)
    g = ctx.basis_ranging(A, b, c, q["basis"], False)
    _same(g, r)
    assert g["status"] == capi.OPTIMAL
    for eps in (0.0, 1e-12):   # ratios of tiny |beta| / |alpha| enter too
        _same(ctx.basis_ranging(A, b, c, q["basis"], False, eps=eps), RR.ranging(A, b, c, q["basis"], False, eps))


def test_degenerate_lp_has_zero_width_ends(ctx):
    """Rows of rhs exactly 0 with a basic variable at level 0: an end equal to b_i itself."""
    found = 0
    for seed in range(12):
        A, b, c, k = lpcases.degenerate_eq_lp(seed)
        q = o.two_phase(A, b, c, False, A.shape[1])
        if q["status"] != o.OPTIMAL:
            continue
        g = ctx.basis_ranging(A, b, c, q["basis"], False)
        _same(g, RR.ranging(A, b, c, q["basis"], False))
        if (g["b_lo"] == b).any() or (g["b_hi"] == b).any():
            found += 1
    assert found >= 1


@pytest.mark.parametrize("m,n", [(40, 100), (300, 600)])
@pytest.mark.parametrize("maximize", [True, False])
def test_nonbasic_cost_ends_are_c_minus_d(ctx, m, n, maximize):
    A, b, c, basis = capi.gen_lp(3 * m, m, n)
    if not maximize:
        c = -c
    s = ctx.simplex_solve(A, b, c, basis, maximize, n)
    g = ctx.basis_ranging(A, b, c, s["basis"], maximize)
    d = ctx.basis_duals(A, b, c, s["basis"])["d"]
    nb = np.setdiff1d(np.arange(n), s["basis"])
    end = g["c_hi"] if maximize else g["c_lo"]
    assert np.array_equal(end[nb].view(np.uint64), (c[nb] - d[nb]).view(np.uint64))
    assert np.array_equal(g["c_enter"][nb, 1 if maximize else 0], nb)
    inf = g["c_lo"] if maximize else g["c_hi"]
    assert np.isinf(inf[nb]).all()
    assert np.array_equal(d, D.duals(A, b, c, s["basis"])["d"])
