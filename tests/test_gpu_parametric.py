"""The parametric right-hand-side path on the GPU (lp_basis_parametric, lp_basis_parametric_batched,
lp_batched_parametric): every breakpoint, value, slope, pivot, final basis, nseg and status bit for bit against
tests/ref/parametric_ref.c, on the batched kernel at both block sizes and both senses, on the single-LP launch path
beyond lp_basis_parametric_fits, after plain, two-phase and re-solve batch runs and on the per-LP fallback."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import lpcases
from tests import parametric_ref as P
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
    A, b, c, basis, d, mx = P.named_cases()[name]
    assert ctx.basis_parametric_fits(*A.shape)
    for t_max in (np.inf, 0.75):
        g = ctx.basis_parametric(A, b, c, basis, d, t_max, mx)
        _same(g, P.trim(P.parametric(A, b, c, basis, d, t_max, mx)))


def test_named_cases_cover_the_outcomes(ctx):
    cases = P.named_cases()
    ns = {k: ctx.basis_parametric(*v[:5], np.inf, v[5]) for k, v in cases.items()}
    assert max(len(r["slope"]) for r in ns.values()) >= 3
    assert ns["infeasible_end"]["status"] == capi.INFEASIBLE
    assert ns["unbounded_t"]["status"] == capi.OPTIMAL and ns["unbounded_t"]["t"][-1] == np.inf
    z = ns["zero_length"]["t"]
    assert (np.diff(z) == 0).any()
    A, b, c, basis, d, mx = cases["max_16x40"]
    full = ns["max_16x40"]
    t_mid = 0.5 * (full["t"][1] + full["t"][2])
    mid = ctx.basis_parametric(A, b, c, basis, d, t_mid, mx)
    assert mid["status"] == capi.OPTIMAL and len(mid["slope"]) == 2 and mid["t"][-1] == t_mid
    lim = ctx.basis_parametric(A, b, c, basis, d, np.inf, mx, max_breaks=2)
    assert lim["status"] == capi.ITER_LIMIT and len(lim["slope"]) == 3 and lim["leave"][-1] >= 0


@pytest.mark.parametrize("m,n,k", [(8, 20, None), (64, 192, None), (6, None, 10), (64, None, 128)])
def test_batched_kernel_both_block_sizes_both_senses(ctx, m, n, k):
    # (m+1)(n+1) <= 4096: 256 threads, else 1024; gen_lp cases are max problems, min_lp ones min problems
    batch = 96
    cases = [P.max_case(s, m, n) if k is None else P.min_case(s, m, k) for s in range(batch)]
    A, b, c, basis, d = _stack(cases)
    mx = k is None
    assert ctx.basis_parametric_fits(m, A.shape[2])
    for t_max, mb in ((np.inf, 64), (0.3, 64), (np.inf, 3)):
        g = ctx.basis_parametric_batched(A, b, c, basis, d, t_max, mx, max_breaks=mb)
        _same(g, P.parametric_batched(A, b, c, basis, d, t_max, mx, max_breaks=mb))


def test_single_lp_beyond_fits_512x1024(ctx):
    m, n = 512, 1024
    assert not ctx.basis_parametric_fits(m, n)
    A, b, c, basis = capi.gen_lp(77, m, n)
    s = ctx.simplex_solve(A, b, c, basis, True, n)
    assert s["status"] == capi.OPTIMAL
    d = P.direction(77, b)
    g = ctx.basis_parametric(A, b, c, s["basis"], d)
    r = P.parametric(A, b, c, s["basis"], d)
    _same(g, P.trim(r))
    assert len(g["slope"]) >= 3


@pytest.mark.parametrize("maximize", [True, False])
def test_just_past_the_predicate(ctx, maximize):
    m = 64
    n = 192
    while ctx.basis_parametric_fits(m, n + 1):
        n += 1
    assert ctx.basis_parametric_fits(m, n) and not ctx.basis_parametric_fits(m, n + 1)
    n += 1
    A, b, c, basis = capi.gen_lp(90 + int(maximize), m, n)
    if not maximize:
        c = -c
    s = ctx.simplex_solve(A, b, c, basis, maximize, n)
    assert s["status"] == capi.OPTIMAL
    d = P.direction(90, b)
    for t_max in (np.inf, 0.4):
        g = ctx.basis_parametric(A, b, c, s["basis"], d, t_max, maximize)
        _same(g, P.trim(P.parametric(A, b, c, s["basis"], d, t_max, maximize)))
    h = ctx.basis_parametric_batched(A[None], b[None], c[None], s["basis"][None], d[None], np.inf, maximize)
    _same(h, P.parametric_batched(A[None], b[None], c[None], s["basis"][None], d[None], np.inf, maximize))


def test_plain_handle_mixed_outcomes_4096(ctx):
    batch, m, n = 4096, 64, 192
    cases = [capi.gen_lp(seed, m, n) for seed in range(batch)]
    A, b, c, basis = (np.stack([k[i] for k in cases]) for i in range(4))
    d = np.stack([P.direction(s, b[s]) for s in range(batch)])
    d[0::4] = -b[0::4]                                   # shrink to 0: long degenerate paths, past max_breaks
    d[1::4] = b[1::4]                                    # scale b: B^-1 d >= 0, the path reaches +inf at once
    p = ctx.batched_problem(A, b, c, basis, True, n - m)
    try:
        assert p.path() == 1
        with pytest.raises(capi.LPError) as e:
            p.parametric(d)   # before the first run
        assert e.value.code == capi.BAD_ARG
        p.run()
        s = p.download()
        g = p.parametric(d, max_breaks=64)
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    r = P.parametric_batched(A, b, c, s["basis"], d, np.inf, True, max_breaks=64, run_status=s["status"])
    _same(g, r)
    for st in (capi.OPTIMAL, capi.INFEASIBLE, capi.ITER_LIMIT):
        assert (g["status"] == st).sum() > 0, st


def test_two_phase_handle(ctx):
    cases = [lpcases.min_lp(seed, 12, 20, negative_rows=4) for seed in range(64)]
    A, b, c = (np.stack([k[i] for k in cases]) for i in range(3))
    d = np.stack([P.direction(s, b[s]) for s in range(64)])
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=32)
    try:
        p.run()
        s = p.download()
        g = p.parametric(d)
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, P.parametric_batched(A, b, c, s["basis"], d, np.inf, False, run_status=s["status"]))


def test_resolve_handle(ctx):
    batch, m, n = 256, 32, 96
    A, b, b2, c, basis = R.scenario(batch, m, n, 500)
    cold = ctx.simplex_solve_batched(A, b, c, basis, True, n - m)
    assert (cold["status"] == capi.OPTIMAL).all()
    d = np.stack([P.direction(s, b2[s]) for s in range(batch)])
    p = ctx.batched_resolve_problem(A, b2, c, cold["basis"], True, n)
    try:
        assert p.path() == 1
        p.run()
        s = p.download()
        g = p.parametric(d, t_max=2.0)
    finally:
        p.free()
    r = P.parametric_batched(A, b2, c, s["basis"], d, 2.0, True, run_status=s["status"])
    _same(g, r)
    assert (g["status"] != capi.BAD_ARG).all()


def test_fallback_handle(ctx):
    cases = [lpcases.min_lp(seed, 136, 136) for seed in range(2)]   # beyond the two-phase and parametric kernels
    A, b, c = (np.stack([k[i] for k in cases]) for i in range(3))
    d = np.stack([P.direction(s, b[s]) for s in range(2)])
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=272)
    try:
        assert p.path() == 0
        p.run()
        s = p.download()
        g = p.parametric(d)
    finally:
        p.free()
    assert (s["status"] == capi.OPTIMAL).all()
    _same(g, P.parametric_batched(A, b, c, s["basis"], d, np.inf, False, run_status=s["status"]))


def test_bad_arguments_and_singular(ctx):
    A, b, c, basis, d, mx = P.named_cases()["max_8x20"]

    def bad(**kw):
        args = dict(A=A, b=b, c=c, basis=basis, d=d, t_max=np.inf, maximize=mx)
        args.update(kw)
        with pytest.raises(capi.LPError) as e:
            ctx.basis_parametric(**args)
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
    assert P.parametric(A, b, c, slack, d, maximize=mx)["status"] == P.BAD_ARG
    rep = basis.copy()
    rep[1] = rep[0]
    g = ctx.basis_parametric(A, b, c, rep, d, np.inf, mx)
    assert g["status"] == capi.SINGULAR and len(g["t"]) == 0 and np.array_equal(g["basis"], rep)
    assert P.parametric(A, b, c, rep, d, maximize=mx)["status"] == P.SINGULAR
    # per LP in a batch: a repeated and a non-optimal basis beside a good one, on both sides of the predicate
    for shape in ((8, 20), (64, 1000)):
        A2, b2, c2, basis2 = capi.gen_lp(5, *shape)
        s = ctx.simplex_solve(A2, b2, c2, basis2, True, shape[1])
        good = s["basis"]
        rep2 = good.copy()
        rep2[1] = rep2[0]
        B = np.stack([good, rep2, basis2])
        AA, bb, cc = np.stack([A2] * 3), np.stack([b2] * 3), np.stack([c2] * 3)
        dd = np.stack([P.direction(5, b2)] * 3)
        g = ctx.basis_parametric_batched(AA, bb, cc, B, dd)
        _same(g, P.parametric_batched(AA, bb, cc, B, dd))
        assert list(g["status"][1:]) == [capi.SINGULAR, capi.BAD_ARG]
        assert (g["nseg"][1:] == 0).all() and np.isnan(g["t"][1:]).all()
