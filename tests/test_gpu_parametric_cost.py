"""The parametric cost path on the GPU (lp_basis_parametric_cost, lp_basis_parametric_cost_batched,
lp_batched_parametric_cost): every breakpoint, value, slope, pivot, final basis, nseg and status bit for bit against
tests/ref/parametric_cost_ref.c, on the batched kernel at both block sizes and both senses, on the single-LP launch
path beyond lp_basis_parametric_cost_fits, after plain, two-phase and re-solve batch runs and on the per-LP
fallback."""
import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import lpcases
from tests import parametric_cost_ref as P
from tests import resolve_ref as R

pytestmark = pytest.mark.gpu


def _same(g, r):
    """Bit for bit (signed zeros included), NaN where the reference has NaN, integers equal."""
    for key in ("status", "nseg", "enter", "leave", "basis"):
        if key in g:
            assert np.array_equal(np.asarray(g[key]), np.asarray(r[key])), key
    for key in P.KEYS:
        a, b = np.asarray(g[key], dtype=np.float64), np.asarray(r[key], dtype=np.float64)
        assert a.shape == b.shape, key
        nan = np.isnan(a)
        assert np.array_equal(nan, np.isnan(b)), key
        assert np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)), key


def _stack(cases):
    return tuple(np.stack([k[i] for k in cases]) for i in range(5))


@pytest.mark.parametrize("name", sorted(P.named_cases()))
def test_named_case_single_lp(ctx, name):
    A, b, c, basis, g, mx = P.named_cases()[name]
    assert ctx.basis_parametric_cost_fits(*A.shape)
    for t_max in (np.inf, 0.75):
        p = ctx.basis_parametric_cost(A, b, c, basis, g, t_max, mx)
        _same(p, P.trim(P.parametric_cost(A, b, c, basis, g, t_max, mx)))


def test_named_cases_cover_the_outcomes(ctx):
    cases = P.named_cases()
    ns = {k: ctx.basis_parametric_cost(*v[:5], np.inf, v[5]) for k, v in cases.items()}
    assert max(len(r["slope"]) for r in ns.values()) >= 3
    for k in ("unbounded_max", "unbounded_min", "min_12x32_unbounded"):
        assert ns[k]["status"] == capi.UNBOUNDED and ns[k]["leave"][-1] == -1 and ns[k]["enter"][-1] >= 0
    assert ns["zero_g"]["status"] == capi.OPTIMAL and len(ns["zero_g"]["slope"]) == 1
    assert ns["zero_g"]["slope"][0] == 0.0 and np.isfinite(ns["zero_g"]["obj"][-1])
    assert ns["max_8x20"]["obj"][-1] == np.inf and ns["min_6x16_inf"]["obj"][-1] == np.inf
    for k in ("zero_length_max", "zero_length_min"):
        assert (np.diff(ns[k]["t"]) == 0).any()
    A, b, c, basis, g, mx = cases["max_16x40"]
    full = ns["max_16x40"]
    t_mid = 0.5 * (full["t"][1] + full["t"][2])
    mid = ctx.basis_parametric_cost(A, b, c, basis, g, t_mid, mx)
    assert mid["status"] == capi.OPTIMAL and len(mid["slope"]) == 2 and mid["t"][-1] == t_mid
    lim = ctx.basis_parametric_cost(A, b, c, basis, g, np.inf, mx, max_breaks=2)
    assert lim["status"] == capi.ITER_LIMIT and len(lim["slope"]) == 3 and lim["enter"][-1] >= 0


@pytest.mark.parametrize("m,n,k", [(8, 20, None), (64, 192, None), (6, None, 10), (64, None, 128)])
def test_batched_kernel_both_block_sizes_both_senses(ctx, m, n, k):
    # (m+1)(n+1) <= 4096: 256 threads, else 1024; gen_lp cases are max problems, min_lp ones min problems
    batch = 96
    cases = [P.max_case(s, m, n) if k is None else P.min_case(s, m, k, positive=s % 2 == 0) for s in range(batch)]
    A, b, c, basis, g = _stack(cases)
    mx = k is None
    assert ctx.basis_parametric_cost_fits(m, A.shape[2])
    for t_max, mb in ((np.inf, 64), (0.3, 64), (np.inf, 3)):
        p = ctx.basis_parametric_cost_batched(A, b, c, basis, g, t_max, mx, max_breaks=mb)
        _same(p, P.parametric_cost_batched(A, b, c, basis, g, t_max, mx, max_breaks=mb))


@pytest.mark.parametrize("maximize", [True, False])
def test_named_cases_batched(ctx, maximize):
    named = [v for v in P.named_cases().values() if v[5] == maximize]
    for A, b, c, basis, g, mx in named:
        p = ctx.basis_parametric_cost_batched(A[None], b[None], c[None], basis[None], g[None], np.inf, mx)
        _same(p, P.parametric_cost_batched(A[None], b[None], c[None], basis[None], g[None], np.inf, mx))


@pytest.mark.parametrize("maximize", [True, False])
def test_single_lp_beyond_fits_128x256(ctx, maximize):
    m, n = 128, 256
    assert not ctx.basis_parametric_cost_fits(m, n)
    if maximize:
        A, b, c, basis, g, mx = P.max_case(81, m, n)
    else:
        A, b, c, basis, g, mx = P.min_case(81, m, n - m)
    for t_max, mb in ((np.inf, 64), (0.2, 64), (np.inf, 5)):
        p = ctx.basis_parametric_cost(A, b, c, basis, g, t_max, mx, max_breaks=mb)
        _same(p, P.trim(P.parametric_cost(A, b, c, basis, g, t_max, mx, max_breaks=mb)))
    assert len(p["slope"]) == 6


def test_single_lp_beyond_fits_unbounded_and_zero_g(ctx):
    A, b, c, basis, g, mx = P.min_case(82, 128, 128)
    p = ctx.basis_parametric_cost(A, b, c, basis, g, np.inf, mx, max_breaks=200)
    r = P.parametric_cost(A, b, c, basis, g, np.inf, mx, max_breaks=200)
    _same(p, P.trim(r))
    assert r["status"] == P.UNBOUNDED
    z = ctx.basis_parametric_cost(A, b, c, basis, np.zeros_like(g), np.inf, mx)
    _same(z, P.trim(P.parametric_cost(A, b, c, basis, np.zeros_like(g), np.inf, mx)))


def test_single_lp_beyond_fits_512x1024(ctx):
    m, n = 512, 1024
    assert not ctx.basis_parametric_cost_fits(m, n)
    A, b, c, basis = capi.gen_lp(77, m, n)
    s = ctx.simplex_solve(A, b, c, basis, True, n)
    assert s["status"] == capi.OPTIMAL
    g = P.direction(77, c)
    p = ctx.basis_parametric_cost(A, b, c, s["basis"], g)
    r = P.parametric_cost(A, b, c, s["basis"], g)
    _same(p, P.trim(r))
    assert len(p["slope"]) >= 3


@pytest.mark.parametrize("maximize", [True, False])
def test_just_past_the_predicate(ctx, maximize):
    m = 64
    n = 192
    while ctx.basis_parametric_cost_fits(m, n + 1):
        n += 1
    assert ctx.basis_parametric_cost_fits(m, n) and not ctx.basis_parametric_cost_fits(m, n + 1)
    n += 1
    A, b, c, basis = capi.gen_lp(90 + int(maximize), m, n)
    if not maximize:
        c = -c
    s = ctx.simplex_solve(A, b, c, basis, maximize, n)
    assert s["status"] == capi.OPTIMAL
    g = P.direction(90, c)
    for t_max in (np.inf, 0.4):
        p = ctx.basis_parametric_cost(A, b, c, s["basis"], g, t_max, maximize)
        _same(p, P.trim(P.parametric_cost(A, b, c, s["basis"], g, t_max, maximize)))
    h = ctx.basis_parametric_cost_batched(A[None], b[None], c[None], s["basis"][None], g[None], np.inf, maximize)
    _same(h, P.parametric_cost_batched(A[None], b[None], c[None], s["basis"][None], g[None], np.inf, maximize))


def _mixed_lp(seed, m=64, n=192):
    """gen_lp with a seeded g; every fourth LP gets a recession column (x0 with A[:, 0] <= 0, costly at t = 0, made
    improving by g_0 > 0), every fourth a g that is non-zero on a few columns only."""
    A, b, c, basis = capi.gen_lp(seed, m, n)
    g = P.direction(seed, c)
    if seed % 4 == 1:
        g = np.where(np.arange(n) % 16 == 0, np.abs(g), 0.0)
    elif seed % 4 == 2:
        A = A.copy()
        A[:, 0] = -A[:, 0]
        c = c.copy()
        c[0] = -50.0
        g = 0.05 * g
        g[0] = 1.0
    return A, b, c, basis, g


def test_plain_handle_mixed_outcomes_4096(ctx):
    batch, m, n = 4096, 64, 192
    A, b, c, basis, g = _stack([_mixed_lp(seed, m, n) for seed in range(batch)])
    p = ctx.batched_problem(A, b, c, basis, True, n - m)
    try:
        assert p.path() == 1
        with pytest.raises(capi.LPError) as e:
            p.parametric_cost(g)   # before the first run
        assert e.value.code == capi.BAD_ARG
        p.run()
        s = p.download()
        pc = p.parametric_cost(g, max_breaks=64)
        rhs = p.parametric(np.zeros((batch, m)), max_breaks=0)
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    r = P.parametric_cost_batched(A, b, c, s["basis"], g, np.inf, True, max_breaks=64, run_status=s["status"])
    _same(pc, r)
    for st in (capi.OPTIMAL, capi.UNBOUNDED, capi.ITER_LIMIT):
        assert (pc["status"] == st).sum() > 0, st
    # the value at t = 0 is the RHS path's, compared as values
    assert np.array_equal(pc["obj"][:, 0], rhs["obj"][:, 0])


def test_two_phase_handle(ctx):
    cases = [lpcases.min_lp(seed, 12, 20, negative_rows=4) for seed in range(64)]
    A, b, c = (np.stack([k[i] for k in cases]) for i in range(3))
    g = np.stack([P.direction(s, c[s]) for s in range(64)])
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=32)
    try:
        p.run()
        s = p.download()
        pc = p.parametric_cost(g)
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(pc, P.parametric_cost_batched(A, b, c, s["basis"], g, np.inf, False, run_status=s["status"]))
    assert (pc["status"] == capi.UNBOUNDED).sum() > 0


def test_resolve_handle(ctx):
    batch, m, n = 256, 32, 96
    A, b, b2, c, basis = R.scenario(batch, m, n, 500)
    cold = ctx.simplex_solve_batched(A, b, c, basis, True, n - m)
    assert (cold["status"] == capi.OPTIMAL).all()
    g = np.stack([P.direction(s, c[s]) for s in range(batch)])
    p = ctx.batched_resolve_problem(A, b2, c, cold["basis"], True, n)
    try:
        assert p.path() == 1
        p.run()
        s = p.download()
        pc = p.parametric_cost(g, t_max=2.0)
    finally:
        p.free()
    r = P.parametric_cost_batched(A, b2, c, s["basis"], g, 2.0, True, run_status=s["status"])
    _same(pc, r)
    assert (pc["status"] != capi.BAD_ARG).all()


def test_fallback_handle(ctx):
    cases = [lpcases.min_lp(seed, 136, 136) for seed in range(2)]   # beyond the two-phase and parametric kernels
    A, b, c = (np.stack([k[i] for k in cases]) for i in range(3))
    g = np.stack([P.direction(s, c[s]) for s in range(2)])
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=272)
    try:
        assert p.path() == 0
        p.run()
        s = p.download()
        pc = p.parametric_cost(g)
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(pc, P.parametric_cost_batched(A, b, c, s["basis"], g, np.inf, False, run_status=s["status"]))


def test_obj0_equals_the_rhs_path(ctx):
    for A, b, c, basis, g, mx in P.named_cases().values():
        pc = ctx.basis_parametric_cost(A, b, c, basis, g, np.inf, mx)
        rhs = ctx.basis_parametric(A, b, c, basis, np.zeros(A.shape[0]), np.inf, mx, max_breaks=0)
        assert pc["obj"][0] == rhs["obj"][0]


def test_bad_arguments_and_singular(ctx):
    A, b, c, basis, g, mx = P.named_cases()["max_8x20"]

    def bad(**kw):
        args = dict(A=A, b=b, c=c, basis=basis, g=g, t_max=np.inf, maximize=mx)
        args.update(kw)
        with pytest.raises(capi.LPError) as e:
            ctx.basis_parametric_cost(**args)
        assert e.value.code == capi.BAD_ARG

    bad(t_max=-1.0)
    bad(t_max=np.nan)
    bad(eps=-1e-9)
    bad(eps=np.nan)
    bad(max_breaks=-1)
    bad(basis=np.where(np.arange(8) == 3, 20, basis))
    bad(basis=np.where(np.arange(8) == 3, -1, basis))
    m, n = A.shape
    slack = np.arange(n - m, n, dtype=np.int32)   # primal feasible, not dual feasible: no valid start
    bad(basis=slack)
    assert P.parametric_cost(A, b, c, slack, g, maximize=mx)["status"] == P.BAD_ARG
    rep = basis.copy()
    rep[1] = rep[0]
    p = ctx.basis_parametric_cost(A, b, c, rep, g, np.inf, mx)
    assert p["status"] == capi.SINGULAR and len(p["t"]) == 0 and np.array_equal(p["basis"], rep)
    assert P.parametric_cost(A, b, c, rep, g, maximize=mx)["status"] == P.SINGULAR
    # per LP in a batch: a repeated and a non-optimal basis beside a good one, on both sides of the predicate
    for shape in ((8, 20), (64, 1000)):
        A2, b2, c2, basis2 = capi.gen_lp(5, *shape)
        s = ctx.simplex_solve(A2, b2, c2, basis2, True, shape[1])
        good = s["basis"]
        rep2 = good.copy()
        rep2[1] = rep2[0]
        B = np.stack([good, rep2, basis2])
        AA, bb, cc = np.stack([A2] * 3), np.stack([b2] * 3), np.stack([c2] * 3)
        gg = np.stack([P.direction(5, c2)] * 3)
        p = ctx.basis_parametric_cost_batched(AA, bb, cc, B, gg)
        _same(p, P.parametric_cost_batched(AA, bb, cc, B, gg))
        assert list(p["status"][1:]) == [capi.SINGULAR, capi.BAD_ARG]
        assert (p["nseg"][1:] == 0).all() and np.isnan(p["t"][1:]).all()


def test_oracle_optimum_is_the_first_value(ctx):
    """obj[0] is the optimum the oracle finds for c (compared as values)."""
    A, b, c, basis = capi.gen_lp(8, 16, 40)
    r = o.simplex_tableau(A, b, c, basis, True, 40)
    p = ctx.basis_parametric_cost(A, b, c, np.asarray(r["basis"], np.int32), P.direction(8, c))
    assert abs(p["obj"][0] - r["obj"]) <= 1e-12 * abs(r["obj"])
