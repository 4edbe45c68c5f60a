"""GPU parity across the tolerance eps: every solve entry against its oracle or CPU reference, bit for bit, at eps
values from 0 to +inf, on the families of tests/tolcases.py (ulp near-ties in the ratio test and the pricing, exact
ties, tiny and huge operands, power-of-two scalings).  tests/test_tolerance_cpu.py checks on the oracle that these
cases do depend on eps, so that agreement here means something.

Floats are compared by their bits (-0.0 is not +0.0), except NaNs: those must sit at the same positions, but their
payloads differ between the host and the device."""
import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import bland_ref, bounded_ref, lpcases, mip_ref, resolve_ref
from tests import tolcases as T

pytestmark = pytest.mark.gpu

ALGOS = [capi.SIMPLEX_LAUNCH, capi.SIMPLEX_LOOKAHEAD, capi.SIMPLEX_RESIDENT, capi.SIMPLEX_OVERLAP, capi.SIMPLEX_AUTO]
COMPOSITE_EPS = (0.0, 1e-12, 1e-2)
BAD_EPS = (-1e-9, -np.inf, np.nan)

_INPUTS = {}
_ORACLE = {}


def _case(fam, seed, m, n, idx):
    key = (fam, seed, m, n, idx)
    if key not in _INPUTS:
        _INPUTS[key] = T.family_case(fam, seed, m, n, idx)
    return _INPUTS[key]


def _oracle(key, A, b, c, basis, eps, max_iter):
    """The oracle's tableau restatement, once per (case, eps bits, max_iter) for every algorithm."""
    k = (key, np.float64(eps).tobytes(), max_iter)
    if k not in _ORACLE:
        m, n = A.shape
        _ORACLE[k] = o.simplex_tableau(A, b, c, basis, True, n - m, eps=eps, max_iter=max_iter, trace_cap=1 << 14,
                                       want_tableau=True)
    return _ORACLE[k]


def _same_bits(a, b):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _run(ctx, A, b, c, basis, eps, max_iter, algo, rule="dantzig"):
    m, n = A.shape
    p = ctx.simplex_problem(A, b, c, basis, True, n - m)
    try:
        if rule != "dantzig":
            p.set_pivot_rule(rule)
        rc, st = p.run(eps=eps, max_iter=max_iter, algo=algo)
        out = p.download(trace_cap=max(st.pivots, 1), want_tableau=True)
    finally:
        p.free()
    assert st.fell_back == 0
    if algo != capi.SIMPLEX_AUTO:
        assert st.algo_used == algo, (st.algo_used, algo)
    out.update(status=rc, iters=st.pivots)
    return out


def _assert_same(g, r, what=""):
    assert g["status"] == r["status"], what
    assert g["iters"] == r["iters"], what
    k = r["iters"]
    assert list(zip(g["trace_enter"][:k].tolist(), g["trace_leave"][:k].tolist())) == r["trace"][:k], what
    assert np.array_equal(g["basis"], r["basis"]), what
    if r["status"] == o.OPTIMAL:
        assert _same_bits(g["x"], r["x"]), what
        assert _same_bits(g["obj"], r["obj"]), what
    if r["status"] in (o.OPTIMAL, o.ITER_LIMIT, o.UNBOUNDED):
        assert _same_bits(g["tableau"], r["tableau"]), what


def _eps_of(case):
    return [e for e in T.EPS_ALL if e != T.LARGE_EPS or case[6]]


# ---- single LP: every algorithm, every family, every shape ---------------------------------------------------------
@pytest.mark.parametrize("case", T.single_cases(), ids=T.case_id)
def test_single_lp_every_algorithm_every_eps(ctx, case):
    fam, seed, m, n, idx, max_iter, _ = case
    A, b, c, basis = _case(fam, seed, m, n, idx)
    key = (fam, seed, m, n, idx)
    for eps in _eps_of(case):
        r = _oracle(key, A, b, c, basis, eps, max_iter)
        if eps == np.inf:
            assert r["iters"] == 0 and r["status"] == o.OPTIMAL   # nothing beats the slack vertex by +inf
        if eps == 0.0 and np.signbit(eps):   # -0.0: the oracle's answer is +0.0's, bit for bit
            r0 = _oracle(key, A, b, c, basis, 0.0, max_iter)
            assert r["trace"] == r0["trace"] and _same_bits(r["tableau"], r0["tableau"])
        for algo in ALGOS:
            g = _run(ctx, A, b, c, basis, eps, max_iter, algo)
            _assert_same(g, r, (eps, algo))


@pytest.mark.parametrize("seed", range(3))
def test_first_pivot_near_ties_on_the_resident_kernel(ctx, seed):
    """The "many small LPs" family: the first ratio test of every LP is an ulp near-tie pair whose row BEHIND the
    first minimum is truly smaller.  At eps = 0 the chain takes it; a ranking by approximate quotients often keeps
    the front row.  One pivot per LP on the chip-resident kernel and AUTO (its default for these shapes)."""
    A, b, c, basis = T.first_pivot_pairs(10 + seed, 64)
    for k in range(A.shape[0]):
        key = ("pairs", seed, k)
        for eps in (0.0, 2.0 ** -60, 1e-12):
            r = _oracle(key, A[k], b[k], c[k], basis[k], eps, 1)
            for algo in (capi.SIMPLEX_RESIDENT, capi.SIMPLEX_AUTO):
                g = _run(ctx, A[k], b[k], c[k], basis[k], eps, 1, algo)
                _assert_same(g, r, (k, eps, algo))


@pytest.mark.parametrize("m,n", [(64, 160), (512, 1024), (768, 1536)])
def test_subnormal_first_pivot_pinned(ctx, m, n):
    """max_iter = 1: the first pivot alone, on a degenerate row whose entering entry is 5e-324 (no finite
    reciprocal), behind the row with the smallest positive ratio, at several offsets."""
    for off in (1, 64, 255, 511):
        A, b, c, basis = T.tiny_entry(21, m, n, 5e-324, off)
        key = ("subnormal", m, n, off)
        for eps in (0.0, -0.0, 1e-300):
            r = _oracle(key, A, b, c, basis, eps, 1)
            assert (r["trace"][0][1] == int(np.flatnonzero(b == 0.0)[0])) == (eps == 0.0)   # (5e-324 > eps)
            for algo in ALGOS:
                _assert_same(_run(ctx, A, b, c, basis, eps, 1, algo), r, (off, eps, algo))


@pytest.mark.parametrize("eps", [0.0, 1e-2])
def test_overlap_2048x4096(ctx, eps):
    m, n = 2048, 4096
    A, b, c, basis = T.near_tie_rows(31, m, n, 512)
    r = _oracle(("overlap", m, n), A, b, c, basis, eps, 40)
    assert r["iters"] > 0
    _assert_same(_run(ctx, A, b, c, basis, eps, 40, capi.SIMPLEX_OVERLAP), r, eps)


@pytest.mark.parametrize("eps", [0.0, 1e-2])
@pytest.mark.parametrize("fam,idx,m,n", [("near_rows", 0, 64, 160), ("near_cols", 0, 64, 160), ("ties", 0, 200, 600),
                                         ("tiny", 1, 64, 160)])
def test_bland_launch(ctx, fam, idx, m, n, eps):
    A, b, c, basis = _case(fam, 5, m, n, idx)
    r = bland_ref.simplex_tableau(A, b, c, basis, True, n - m, rule=bland_ref.BLAND, eps=eps, trace_cap=1 << 14,
                                  want_tableau=True)
    g = _run(ctx, A, b, c, basis, eps, capi.MAX_ITER, capi.SIMPLEX_LAUNCH, rule="bland")
    _assert_same(g, r, eps)


# ---- metamorphic: power-of-two scalings at eps = 0 ----------------------------------------------------------------
def _assert_scaled(s, r, kb, kc):
    assert s["status"] == r["status"] == o.OPTIMAL and r["iters"] > 0
    assert s["iters"] == r["iters"]
    assert np.array_equal(s["basis"], r["basis"])
    if "trace_enter" in r:
        assert np.array_equal(s["trace_enter"], r["trace_enter"]) and np.array_equal(s["trace_leave"], r["trace_leave"])
    assert _same_bits(s["x"], np.asarray(r["x"]) * 2.0 ** kb)
    assert _same_bits(s["obj"], np.asarray(r["obj"]) * 2.0 ** (kb + kc))


@pytest.mark.parametrize("kb,kc", T.POW2)
@pytest.mark.parametrize("algo", [capi.SIMPLEX_RESIDENT, capi.SIMPLEX_LAUNCH])
def test_pow2_scaling_single(ctx, algo, kb, kc):
    """kb > 0 puts every resident ratio above its cap, kb < 0 every xB below the fast reciprocal's range; kc = +-600
    puts the reduced costs outside [2^-500, 2^501), where the pivot quotients take the plain division."""
    for fam, idx, m, n in (("near_rows", 0, 64, 160), ("near_cols", 5, 512, 1024)):
        A, b, c, basis = _case(fam, 3, m, n, idx)
        r = _run(ctx, A, b, c, basis, 0.0, capi.MAX_ITER, algo)
        A2, b2, c2 = T.pow2_scaled(A, b, c, kb, kc)
        s = _run(ctx, A2, b2, c2, basis, 0.0, capi.MAX_ITER, algo)
        _assert_scaled(s, r, kb, kc)


@pytest.mark.parametrize("kb,kc", T.POW2)
def test_pow2_scaling_batched(ctx, kb, kc):
    m, n = 64, 160
    cases = [_case(f, 3, m, n, i) for f, i in (("near_rows", 0), ("near_cols", 5), ("ties", 0))]
    A, b, c, basis = (np.stack(v) for v in zip(*cases))
    r = ctx.simplex_solve_batched(A, b, c, basis, True, n - m, eps=0.0)
    s = ctx.simplex_solve_batched(A, b * 2.0 ** kb, c * 2.0 ** kc, basis, True, n - m, eps=0.0)
    for k in range(A.shape[0]):
        _assert_scaled({key: v[k] for key, v in s.items()}, {key: v[k] for key, v in r.items()}, kb, kc)


# ---- batched and composite entries --------------------------------------------------------------------------------
def _mixed(m, n, seed=7):
    picks = (("near_rows", 0), ("near_rows", 6), ("near_cols", 5), ("ties", 0), ("tiny", 1), ("tiny", 3), ("huge", 0))
    cases = [_case(f, seed, m, n, i) for f, i in picks]
    return (np.stack(v) for v in zip(*cases))


def _assert_lp(g, k, r, what):
    assert g["status"][k] == r["status"], what
    assert np.array_equal(g["basis"][k], r["basis"]), what
    if r["status"] == o.OPTIMAL:
        assert _same_bits(g["x"][k], r["x"]), what
        assert _same_bits(g["obj"][k], r["obj"]), what


@pytest.mark.parametrize("eps", COMPOSITE_EPS)
@pytest.mark.parametrize("m,n", [(64, 160), (200, 600)])   # the LDS kernel; the per-LP fallback (AUTO, resident)
def test_batched(ctx, m, n, eps):
    A, b, c, basis = _mixed(m, n)
    g = ctx.simplex_solve_batched(A, b, c, basis, True, n - m, eps=eps)
    for k in range(A.shape[0]):
        r = _oracle(("batched", m, n, k), A[k], b[k], c[k], basis[k], eps, capi.MAX_ITER)
        assert g["iters"][k] == r["iters"], k
        _assert_lp(g, k, r, (k, eps))


@pytest.mark.parametrize("eps", COMPOSITE_EPS)
def test_batched_bland(ctx, eps):
    m, n = 64, 160
    A, b, c, basis = _mixed(m, n)
    g = ctx.simplex_solve_batched(A, b, c, basis, True, n - m, eps=eps, pivot_rule="bland")
    for k in range(A.shape[0]):
        r = bland_ref.simplex_tableau(A[k], b[k], c[k], basis[k], True, n - m, rule=bland_ref.BLAND, eps=eps)
        assert g["iters"][k] == r["iters"], k
        _assert_lp(g, k, r, (k, eps))


def _two_phase_form(A, b, c):
    """The family LPs without their basis, some rows negated (b < 0: the two-phase row flip)."""
    A, b = A.copy(), b.copy()
    A[..., ::5, :] *= -1.0
    b[..., ::5] *= -1.0
    return A, b, c


@pytest.mark.parametrize("eps", COMPOSITE_EPS)
def test_two_phase_and_batched(ctx, eps):
    m, n = 32, 96
    A, b, c, _ = _mixed(m, n)
    A, b, c = _two_phase_form(A, b, c)
    gb = ctx.two_phase_batched(A, b, c, True, n - m, eps=eps)
    for k in range(A.shape[0]):
        r = o.two_phase(A[k], b[k], c[k], True, n - m, eps=eps)
        g = ctx.two_phase(A[k], b[k], c[k], True, n - m, eps=eps)
        assert g["status"] == r["status"] and g["iters"] == r["iters"], (k, eps)
        assert np.array_equal(g["basis"], r["basis"]), (k, eps)
        if r["status"] == o.OPTIMAL:
            assert _same_bits(g["x"], r["x"]) and _same_bits(g["obj"], r["obj"]), (k, eps)
        assert gb["iters"][k].tolist() == r["iters"], (k, eps)
        _assert_lp(gb, k, r, (k, eps))


def _resolve_start(A, b, c):
    """Dual feasible, primal infeasible at the slack basis for half the LPs (negated costs, some rows' original part
    and b negated: xB < 0 there), the family's primal feasible start for the others."""
    A, b, c = A.copy(), b.copy(), c.copy()
    m, n = A.shape[1:]
    A[1::2, ::3, : n - m] *= -1.0
    b[1::2, ::3] *= -1.0
    c[1::2] = -np.abs(c[1::2])
    return A, b, c


@pytest.mark.parametrize("eps", COMPOSITE_EPS)
def test_resolve_and_batched(ctx, eps):
    m, n = 64, 160
    A, b, c, basis = _mixed(m, n)
    A, b, c = _resolve_start(A, b, c)
    gb = ctx.resolve_batched(A, b, c, basis, True, n - m, eps=eps)
    for k in range(A.shape[0]):
        r = resolve_ref.resolve(A[k], b[k], c[k], basis[k], True, n - m, eps=eps)
        g = ctx.simplex_resolve(A[k], b[k], c[k], basis[k], True, n - m, eps=eps)
        assert g["status"] == r["status"] and g["iters"] == r["iters"], (k, eps)
        assert np.array_equal(g["basis"], r["basis"]), (k, eps)
        if r["status"] == o.OPTIMAL:
            assert _same_bits(g["x"], r["x"]) and _same_bits(g["obj"], r["obj"]), (k, eps)
        assert tuple(gb["iters"][k].tolist()) == r["iters"], (k, eps)
        _assert_lp(gb, k, r, (k, eps))


@pytest.mark.parametrize("eps", COMPOSITE_EPS)
def test_bounded_batched(ctx, eps):
    m, n = 16, 48
    A, b, c, _ = _mixed(m, n)
    A, b, c = _two_phase_form(A, b, c)
    rng = np.random.default_rng(5)
    lo = np.zeros(c.shape)
    hi = np.where(rng.random(c.shape) < 0.5, np.inf, rng.uniform(0.5, 4.0, c.shape))
    hi[:, n - m:] = np.inf   # (slacks unbounded: every LP feasible)
    g = ctx.bounded_batched(A, b, c, lo, hi, True, n - m, eps=eps)
    for k in range(A.shape[0]):
        r = bounded_ref.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n - m, eps=eps)
        assert g["status"][k] == r["status"] and g["iters"][k].tolist() == r["iters"], (k, eps)
        assert np.array_equal(g["basis"][k], r["basis"]) and np.array_equal(g["at_upper"][k], r["at_upper"]), (k, eps)
        assert _same_bits(g["x"][k], r["x"]) and _same_bits(g["obj"][k], r["obj"]), (k, eps)


@pytest.mark.parametrize("eps", COMPOSITE_EPS)
def test_mip_batched(ctx, eps):
    m, n = 8, 24
    A, b, c, basis = _mixed(m, n)
    integer = np.r_[np.arange(n - m) % 2, np.zeros(m)].astype(np.int32)
    g = ctx.mip_batched(A, b, c, basis, integer, True, n - m, eps=eps, max_depth=12, max_nodes=300)
    for k in range(A.shape[0]):
        r = mip_ref.mip(A[k], b[k], c[k], basis[k], integer, True, n - m, eps=eps, max_depth=12, max_nodes=300)
        assert g["status"][k] == r["status"] and g["found"][k] == r["found"], (k, eps)
        assert tuple(g["stats"][k].tolist()) == r["stats"], (k, eps)
        assert _same_bits(g["x"][k], r["x"]) and _same_bits(g["obj"][k], r["obj"]), (k, eps)
        assert _same_bits(g["bound"][k], r["bound"]), (k, eps)


# ---- the domain of eps ----------------------------------------------------------------------------------------------
def _bad_arg(fn):
    with pytest.raises(capi.LPError) as ei:
        fn()
    assert ei.value.code == capi.BAD_ARG


@pytest.mark.parametrize("eps", BAD_EPS, ids=["neg", "neginf", "nan"])
def test_every_solve_entry_refuses_eps_outside_its_domain(ctx, eps):
    m, n = 8, 24
    A, b, c, basis = lpcases.random_lp(3, m, n)
    no = n - m
    AB, bB, cB, basisB = (np.stack([v, v]) for v in (A, b, c, basis))
    lo, hi = np.zeros(n), np.full(n, np.inf)
    integer = np.r_[np.ones(no), np.zeros(m)].astype(np.int32)
    _bad_arg(lambda: ctx.simplex_solve(A, b, c, basis, True, no, eps=eps))
    _bad_arg(lambda: ctx.simplex_solve(A, b, c, basis, True, no, eps=eps, pivot_rule="bland"))
    _bad_arg(lambda: ctx.simplex_resolve(A, b, c, basis, True, no, eps=eps))
    _bad_arg(lambda: ctx.resolve_batched(AB, bB, cB, basisB, True, no, eps=eps))
    _bad_arg(lambda: ctx.two_phase(A, b, c, True, no, eps=eps))
    _bad_arg(lambda: ctx.two_phase(A, b, c, True, no, eps=eps, pivot_rule="bland"))
    _bad_arg(lambda: ctx.two_phase_batched(AB, bB, cB, True, no, eps=eps))
    _bad_arg(lambda: ctx.two_phase_batched(AB, bB, cB, True, no, eps=eps, pivot_rule="bland"))
    _bad_arg(lambda: ctx.simplex_solve_batched(AB, bB, cB, basisB, True, no, eps=eps))
    _bad_arg(lambda: ctx.simplex_solve_batched(AB, bB, cB, basisB, True, no, eps=eps, pivot_rule="bland"))
    _bad_arg(lambda: ctx.bounded(A, b, c, lo, hi, True, no, eps=eps))
    _bad_arg(lambda: ctx.bounded_batched(AB, bB, cB, np.stack([lo, lo]), np.stack([hi, hi]), True, no, eps=eps))
    _bad_arg(lambda: ctx.mip(A, b, c, basis, integer, True, no, eps=eps))
    _bad_arg(lambda: ctx.mip_batched(AB, bB, cB, basisB, integer, True, no, eps=eps))
    # the handles
    p = ctx.simplex_problem(A, b, c, basis, True, no)
    try:
        for algo in ALGOS:
            _bad_arg(lambda: p.run(eps=eps, algo=algo))
        _bad_arg(lambda: p.resolve(eps=eps))
        rc, _ = p.run()   # the handle is still usable
        assert rc == capi.OPTIMAL
    finally:
        p.free()
    for resolve in (False, True):
        bp = ctx.batched_resolve_problem(AB, bB, cB, basisB, True, no) if resolve else \
            ctx.batched_problem(AB, bB, cB, basisB, True, no)
        try:
            _bad_arg(lambda: bp.run(eps=eps))
            bp.run()
            _bad_arg(lambda: bp.mip(integer, eps=eps))
        finally:
            bp.free()
    tp = ctx.batched_two_phase_problem(AB, bB, cB, True, no)
    try:
        _bad_arg(lambda: tp.run(eps=eps))
    finally:
        tp.free()
