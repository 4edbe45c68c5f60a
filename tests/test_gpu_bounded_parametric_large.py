"""The parametric right-hand-side and cost paths of a bounded-variable LP beyond one workgroup's LDS
(lp_basis_bounded_parametric_large, lp_basis_bounded_parametric_cost_large): every output equals
tests/ref/bounded_parametric_ref.c's bit for bit (NaN and -1 fills, signed zeros, side and at_upper included) on every
case of tests/bounded_parametric_large_cases.py (what each case exercises is asserted in
tests/test_bounded_parametric_large_cpu.py), at what ctx.bounded_large and ctx.bounded_resolve_large return, and on the
named small cases with every status; at a shape that fits it equals the LDS entry's, and without bounds the plain HBM
path's; the eps edges move the first leave as the reference says; the refusals are the LDS entry's, and the context
stays usable after each.  The new entries are called through the C ABI with the outputs pre-filled, so that the fills
past the path are the library's."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_large_cases as Q
from tests import bounded_parametric_large_cases as L
from tests import bounded_parametric_ref as R
from tests import bounded_resolve_ref as W

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def _fn(ctx, path):
    return ctx.lib.lp_basis_bounded_parametric_large if path == "rhs" else ctx.lib.lp_basis_bounded_parametric_cost_large


def _large(ctx, path, A, b, c, lo, hi, basis, at_upper, direction, maximize, t_max=np.inf, eps=1e-9, max_breaks=64):
    """The C entry with every output pre-filled with a value no fill uses: the padded dict of R.parametric()."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Af = capi.colmajor(A)
    f = [np.ascontiguousarray(v, np.float64) for v in (b, c, lo, hi, direction)]
    basis, at_upper = np.ascontiguousarray(basis, np.int32), np.ascontiguousarray(at_upper, np.int32)
    nb = max(int(max_breaks), 0)
    t, obj, slope = np.full(nb + 2, 7.0), np.full(nb + 2, 7.0), np.full(nb + 1, 7.0)
    enter, leave, side = (np.full(nb + 1, 77, np.int32) for _ in range(3))
    bo, uo, nseg = np.full(m, 77, np.int32), np.full(n, 77, np.int32), np.full(1, 77, np.int32)
    dp, ip = capi._d, capi._i
    st = _fn(ctx, path)(ctx.h, dp(Af), m, n, dp(f[0]), dp(f[1]), dp(f[2]), dp(f[3]), ip(basis), ip(at_upper),
                        int(maximize), dp(f[4]), float(t_max), float(eps), int(max_breaks), ip(nseg), dp(t), dp(obj),
                        dp(slope), ip(enter), ip(leave), ip(side), ip(bo), ip(uo))
    return dict(status=st, nseg=int(nseg[0]), t=t, obj=obj, slope=slope, enter=enter, leave=leave, side=side, basis=bo,
                at_upper=uo)


def _same(got, want):
    assert int(got["status"]) == int(want["status"])
    R.same_bits(got, want)


def _case(ctx, path, cs, **kw):
    return _large(ctx, path, *cs[:8], cs[8], **kw)


@pytest.mark.parametrize("name,path,make,mb", L.all_cases(), ids=[c[0] for c in L.all_cases()])
def test_every_case_equals_the_reference(ctx, name, path, make, mb):
    cs = make()
    want = L.ref(("tall", name.endswith("reversed")) if name.startswith("tall") else name, path, cs, max_breaks=mb)
    _same(_case(ctx, path, cs, max_breaks=mb), want)
    assert want["nseg"] > 40


@pytest.mark.parametrize("path", L.PATHS)
def test_end_to_end_after_bounded_large(ctx, path):
    m, n, seed = 160, 320, 1
    A, b, c, lo, hi, mx = Q.boxed(m, n, "mixed", seed)
    sol = ctx.bounded_large(A, b, c, lo, hi, mx)
    assert sol["status"] == OPTIMAL
    direction = L.beyond(path, m, n, seed, mx)[7]
    at = (A, b, c, lo, hi, sol["basis"], sol["at_upper"], direction)
    want = R.parametric(path, *at, maximize=mx, max_breaks=L.BEYOND_BREAKS)
    _same(_large(ctx, path, *at, mx, max_breaks=L.BEYOND_BREAKS), want)
    call = ctx.bounded_parametric_large if path == "rhs" else ctx.bounded_parametric_cost_large
    R.same_bits(call(*at, maximize=mx, max_breaks=L.BEYOND_BREAKS), R.trim(want))
    assert want["nseg"] > 40


def test_end_to_end_after_bounded_resolve_large(ctx):
    m, n, seed = 160, 320, 1
    A, b, c, lo, hi, mx = Q.boxed(m, n, "mixed", seed)
    cold = Q.ref(("bpar-large", m, n, seed), A, b, c, lo, hi, mx, n)
    assert cold["status"] == OPTIMAL
    b2, c2, lo2, hi2 = W.perturb(seed, "bound", b, c, lo, hi, cold["basis"], cold["x"])   # a tightened bound
    sol = ctx.bounded_resolve_large(A, b2, c2, lo2, hi2, cold["basis"], cold["at_upper"], mx)
    assert sol["status"] == OPTIMAL and sol["iters"][0] > 0
    for path in L.PATHS:
        direction = L.beyond(path, m, n, seed, mx)[7]
        at = (A, b2, c2, lo2, hi2, sol["basis"], sol["at_upper"], direction)
        want = R.parametric(path, *at, maximize=mx, max_breaks=L.BEYOND_BREAKS)
        _same(_large(ctx, path, *at, mx, max_breaks=L.BEYOND_BREAKS), want)
        assert want["nseg"] > 10


@pytest.mark.parametrize("path", L.PATHS)
def test_against_the_lds_entry(ctx, path):
    m, n = 67, 201
    fits = ctx.bounded_parametric_fits if path == "rhs" else ctx.bounded_parametric_cost_fits
    lds = ctx.bounded_parametric if path == "rhs" else ctx.bounded_parametric_cost
    assert fits(m, n) and not fits(160, 320)
    for key in L.BEYOND:
        if key[:3] != (path, m, n):
            continue
        cs = L.beyond(*key)
        got = _case(ctx, path, cs, max_breaks=L.BEYOND_BREAKS)
        R.same_bits(R.trim(got), lds(*cs[:8], maximize=cs[8], max_breaks=L.BEYOND_BREAKS))
        _same(got, L.ref(L.key_id(key), path, cs))
    cs = L.beyond(path, 160, 320, 1, True)
    with pytest.raises(capi.LPError) as e:
        lds(*cs[:8], maximize=cs[8])
    assert e.value.code == BAD_ARG


@pytest.mark.parametrize("path", L.PATHS)
def test_without_bounds_it_is_the_plain_hbm_path(ctx, path):
    m, n = 160, 320
    plain = ctx.basis_parametric if path == "rhs" else ctx.basis_parametric_cost
    lo, hi, up = np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32)
    walked = 0
    for seed, mx in ((1, True), (2, False)):
        A, b, c, _, _, _ = Q.boxed(m, n, "mixed", seed, mx)
        cold = Q.ref(("bpar-large-plain", m, n, seed, mx), A, b, c, lo, hi, mx)
        if cold["status"] != OPTIMAL:
            continue
        direction = L.beyond(path, m, n, seed, mx)[7]
        at = (A, b, c, lo, hi, cold["basis"], up, direction)
        got = _large(ctx, path, *at, mx, max_breaks=L.BEYOND_BREAKS)
        _same(got, R.parametric(path, *at, maximize=mx, max_breaks=L.BEYOND_BREAKS))
        want = plain(A, b, c, cold["basis"], direction, np.inf, mx, max_breaks=L.BEYOND_BREAKS)
        trimmed = R.trim(got)
        R.same_bits(trimmed, want)
        assert (trimmed["side"][trimmed["leave"] >= 0] == 0).all() and (trimmed["side"][trimmed["leave"] < 0] == -1).all()
        assert not got["at_upper"].any()
        walked += got["nseg"] > 3
    assert walked >= 1


def test_named_small_cases(ctx):
    statuses = set()
    for name, (path, args, kw, status) in sorted(R.named_cases().items()):
        at, mx = args[:8], args[8]
        want = R.parametric(path, *at, maximize=mx, **kw)
        assert status is None or want["status"] == status, name
        got = _large(ctx, path, *at, mx, **kw)
        _same(got, want)
        statuses.add(int(want["status"]))
        if name in ("crossed", "cost_crossed", "singular", "cost_singular", "start_dual_infeasible",
                    "start_primal_infeasible"):
            assert got["nseg"] == 0 and np.isnan(got["t"]).all() and np.isnan(got["obj"]).all(), name
            assert np.isnan(got["slope"]).all(), name
            assert (got["enter"] == -1).all() and (got["leave"] == -1).all() and (got["side"] == -1).all(), name
            assert np.array_equal(got["basis"], at[5]) and np.array_equal(got["at_upper"], at[6]), name
    assert statuses == {OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG}
    for path, name, case, boxed in R.plain_named_cases():
        for t_max, max_breaks in ((np.inf, 64), (0.3, 64), (np.inf, 3)):
            want = R.parametric(path, *boxed[:8], t_max=t_max, maximize=boxed[8], max_breaks=max_breaks)
            _same(_large(ctx, path, *boxed[:8], boxed[8], t_max=t_max, max_breaks=max_breaks), want)


def test_eps_edges_on_the_in_order_tall_rhs_case(ctx):
    cs = L.tall("rhs", False)
    firsts = []
    for eps in (0.0, np.nextafter(8.0, 0.0), 8.0):
        want = L.ref(("tall", False), "rhs", cs, eps=eps, max_breaks=L.TALL_BREAKS)
        _same(_case(ctx, "rhs", cs, eps=eps, max_breaks=L.TALL_BREAKS), want)
        firsts.append(int(want["leave"][0]))
    assert firsts[1] != firsts[2]


def _changed(v, at, val):
    v = np.array(v)
    v[at] = val
    return v


@pytest.fixture(scope="module")
def good_160():
    return {path: (L.beyond(path, 160, 320, 1, True), L.ref(L.key_id((path, 160, 320, 1, True, "mixed")), path,
                                                           L.beyond(path, 160, 320, 1, True))) for path in L.PATHS}


def _good_call(ctx, good_160, path):
    cs, want = good_160[path]
    _same(_case(ctx, path, cs, max_breaks=L.BEYOND_BREAKS), want)


@pytest.mark.parametrize("path", L.PATHS)
def test_refusals_at_160x320(ctx, good_160, path):
    cs, _ = good_160[path]
    A, b, c, lo, hi, basis, up, direction, mx = cs
    n = A.shape[1]
    free = int(np.flatnonzero(np.isinf(hi))[0])
    refusals = [dict(lo=_changed(lo, 0, np.nan)), dict(lo=_changed(lo, 0, -np.inf)), dict(lo=_changed(lo, 0, np.inf)),
                dict(hi=_changed(hi, 0, np.nan)),
                dict(up=_changed(up, 0, 2)), dict(up=_changed(np.zeros(n, np.int32), free, 1)),
                dict(basis=_changed(basis, 1, -1)), dict(basis=_changed(basis, 1, n)),
                dict(t_max=-1.0), dict(t_max=float("nan")), dict(eps=-1e-12), dict(eps=float("nan")),
                dict(max_breaks=-1)]
    for kw in refusals:
        a = dict(lo=lo, hi=hi, basis=basis, up=up, t_max=np.inf, eps=1e-9, max_breaks=8)
        a.update(kw)
        at = (A, b, c, a["lo"], a["hi"], a["basis"], a["up"], direction)
        opts = dict(t_max=a["t_max"], eps=a["eps"], max_breaks=a["max_breaks"])
        assert R.parametric(path, *at, maximize=mx, **opts)["status"] == BAD_ARG, kw
        assert _large(ctx, path, *at, mx, **opts)["status"] == BAD_ARG, kw
        call = ctx.bounded_parametric_large if path == "rhs" else ctx.bounded_parametric_cost_large
        with pytest.raises(capi.LPError) as e:
            call(*at, maximize=mx, **opts)
        assert e.value.code == BAD_ARG, kw
    _good_call(ctx, good_160, path)


@pytest.mark.parametrize("path", L.PATHS)
def test_null_pointers_are_refused(ctx, good_160, path):
    cs, want = good_160[path]
    A, b, c, lo, hi, basis, up, direction, mx = cs
    m, n = A.shape
    mb = L.BEYOND_BREAKS
    Af = capi.colmajor(A)
    f = [np.ascontiguousarray(v, np.float64) for v in (b, c, lo, hi, direction)]
    basis, up = np.ascontiguousarray(basis, np.int32), np.ascontiguousarray(up, np.int32)
    t, obj, slope = np.zeros(mb + 2), np.zeros(mb + 2), np.zeros(mb + 1)
    enter, leave, side = (np.zeros(mb + 1, np.int32) for _ in range(3))
    bo, uo, nseg = np.zeros(m, np.int32), np.zeros(n, np.int32), np.zeros(1, np.int32)
    dp, ip = capi._d, capi._i
    args = [ctx.h, dp(Af), m, n, dp(f[0]), dp(f[1]), dp(f[2]), dp(f[3]), ip(basis), ip(up), int(mx), dp(f[4]), np.inf,
            1e-9, mb, ip(nseg), dp(t), dp(obj), dp(slope), ip(enter), ip(leave), ip(side), ip(bo), ip(uo)]
    fn = _fn(ctx, path)
    for k in (0, 1, 4, 5, 6, 7, 8, 9, 11, 15, 16, 17, 18, 19, 20, 21, 22, 23):
        bad = list(args)
        bad[k] = None
        assert fn(*bad) == BAD_ARG, k
    assert fn(*args) == want["status"]   # the full call is good, and the context still is
    got = dict(status=want["status"], nseg=int(nseg[0]), t=t, obj=obj, slope=slope, enter=enter, leave=leave, side=side,
               basis=bo, at_upper=uo)
    _same(got, want)
