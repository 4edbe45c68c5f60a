"""Farkas and unbounded-ray certificates of a bounded-variable LP beyond one workgroup's LDS
(lp_basis_bounded_certificate_large): every output equals tests/ref/bounded_certificate_ref.c's bit for bit (NaN where it
has NaN, signed zeros included) on every case of tests/bounded_certificate_large_cases.py (what each case exercises is
asserted in tests/test_bounded_certificate_large_cpu.py) and at what ctx.bounded_large and ctx.bounded_resolve_large
return; at a shape that fits it equals the LDS entry's, and without bounds the plain HBM path's (ctx.basis_certificate);
the eps edges move the winner as the reference says; the statuses and the refusals are the LDS entry's, and the context
stays usable after each."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_certcases as BC
from tests import bounded_certificate_large_cases as L
from tests import bounded_certificate_ref as CR
from tests import bounded_large_cases as Q

pytestmark = pytest.mark.gpu

OPTIMAL, SINGULAR, INFEASIBLE, BAD_ARG = L.OPTIMAL, L.SINGULAR, L.INFEASIBLE, L.BAD_ARG


def _same(got, want):
    assert int(got["status"]) == int(want["status"])
    CR.same_bits(got, want)


def _large(ctx, cs, eps=1e-9, maximize=None):
    return ctx.basis_bounded_certificate_large(*L.at(cs), cs["maximize"] if maximize is None else maximize, eps)


@pytest.mark.parametrize("name,make", L.all_cases(), ids=[k for k, _ in L.all_cases()])
def test_every_case_equals_the_reference(ctx, name, make):
    cs = make()
    want = L.ref(name, cs)
    got = _large(ctx, cs)
    _same(got, want)
    BC.check(cs, got)
    if "expect" in cs:
        assert (got["kind"], got["index"], got["value"]) == tuple(cs["expect"][k] for k in ("kind", "index", "value"))


@pytest.mark.parametrize("key", L.TIE_DUAL, ids=str)
def test_tie_dual_eps_edges(ctx, key):
    cs = L.tie_dual(*key)
    t1, _, t3, _ = cs["expect"]["t"]
    for eps, index in ((0.0, t3), (np.nextafter(L.SPOIL, 0.0), t3), (L.SPOIL, t1)):
        want = L.ref(("tie_dual",) + key, cs, eps)
        assert want["index"] == index
        _same(_large(ctx, cs, eps), want)


@pytest.mark.parametrize("key", L.TIE_RAY, ids=str)
def test_tie_ray_eps_edges_and_the_other_sense(ctx, key):
    cs = L.tie_ray(*key)
    _, _, j3, j4 = cs["expect"]["j"]
    for eps, index in ((0.0, j3), (np.nextafter(3.0, 0.0), j3), (3.0, j4)):
        want = L.ref(("tie_ray",) + key, cs, eps)
        assert want["index"] == index
        _same(_large(ctx, cs, eps), want)
    other = not cs["maximize"]
    _same(_large(ctx, cs, 0.0, other), L.ref(("tie_ray",) + key, cs, 0.0, other))


E2E = {"cold-infeasible": lambda: L.cold("infeasible", 160, 320, 1), "cold-unbounded": lambda: L.cold("unbounded", 160, 320, 1),
       "rich": lambda: L.rich(160, 320, 1), "contra": lambda: L.contra(160, 320, 1)}


@pytest.mark.parametrize("name", list(E2E))
def test_end_to_end_after_bounded_large(ctx, name):
    cs = E2E[name]()
    A, b, c, lo, hi = (cs[k] for k in ("A", "b", "c", "lo", "hi"))
    sol = ctx.bounded_large(A, b, c, lo, hi, cs["maximize"])
    assert sol["status"] == cs["run"] and cs["run"] in (L.INFEASIBLE, L.UNBOUNDED)
    assert np.array_equal(sol["basis"], cs["basis"]) and np.array_equal(sol["at_upper"], cs["at_upper"])
    got = ctx.basis_bounded_certificate_large(A, b, c, lo, hi, sol["basis"], sol["at_upper"], cs["maximize"])
    _same(got, L.ref(("e2e", name), cs))
    assert got["kind"] != L.NONE
    BC.check(cs, got)


def test_end_to_end_after_bounded_resolve_large(ctx):
    key = (160, 320, 1, "raise", "above")
    cs = L.unreach(*key)
    A, b, c, lo, hi, mx = Q.boxed(160, 320, "mixed", 1)
    cold = Q.ref(("cert-large", 160, 320, 1), A, b, c, lo, hi, mx)
    assert np.array_equal(A, cs["A"]) and mx == cs["maximize"]
    sol = ctx.bounded_resolve_large(A, b, c, cs["lo"], cs["hi"], cold["basis"], cold["at_upper"], mx)
    assert sol["status"] == INFEASIBLE
    assert np.array_equal(sol["basis"], cs["basis"]) and np.array_equal(sol["at_upper"], cs["at_upper"])
    got = ctx.basis_bounded_certificate_large(A, b, c, cs["lo"], cs["hi"], sol["basis"], sol["at_upper"], mx)
    _same(got, L.ref(("unreach",) + key, cs))
    assert got["kind"] == L.FARKAS and got["index"] >= 0
    BC.check(cs, got)


def test_against_the_lds_entry(ctx):
    m, n = 67, 201
    assert ctx.basis_bounded_certificate_fits(m, n)
    cases = [L.contra(m, n, 1), L.unreach(m, n, 2, "raise", "above"), L.rich(m, n, 1)]
    kinds = []
    for cs in cases:
        got = _large(ctx, cs)
        _same(got, ctx.basis_bounded_certificate(*L.at(cs), cs["maximize"]))
        _same(got, CR.certificate(*L.at(cs), cs["maximize"]))
        kinds.append((got["kind"], got["index"] >= 0 if got["kind"] == L.FARKAS else None))
    assert kinds == [(L.FARKAS, False), (L.FARKAS, True), (L.RAY, None)]   # a phase-I, a dual and a ray case
    cs = L.contra(160, 320, 1)
    assert not ctx.basis_bounded_certificate_fits(160, 320)
    with pytest.raises(capi.LPError) as e:
        ctx.basis_bounded_certificate(*L.at(cs), cs["maximize"])
    assert e.value.code == BAD_ARG


def test_without_bounds_it_is_the_plain_hbm_certificate(ctx):
    m, n = 160, 320
    lo, hi, up = np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32)
    kinds = set()
    for cs in (L.contra(m, n, 1), L.cold("infeasible", m, n, 1), L.rich(m, n, 1), L.cold("unbounded", m, n, 1)):
        A, b, c, basis, mx = cs["A"], cs["b"], cs["c"], cs["basis"], cs["maximize"]
        for maximize in (mx, not mx):
            got = ctx.basis_bounded_certificate_large(A, b, c, lo, hi, basis, up, maximize)
            _same(got, ctx.basis_certificate(A, b, c, basis, maximize))
            _same(got, CR.certificate(A, b, c, lo, hi, basis, up, maximize))
            kinds.add(((np.asarray(basis) >= n).any(), got["kind"]))
    # a phase-I basis and a basis without artificials were both computed (the kinds are whatever the plain entry says)
    assert {k[0] for k in kinds} == {True, False}


def _changed(v, at, val):
    v = np.array(v)
    v[at] = val
    return v


@pytest.fixture(scope="module")
def dual_160():
    key = (160, 320, 1, "raise", "above")
    cs = L.unreach(*key)
    return cs, L.ref(("unreach",) + key, cs)


def _good_call(ctx, dual_160):
    cs, want = dual_160
    _same(_large(ctx, cs), want)


def test_statuses_at_160x320(ctx, dual_160):
    cs, _ = dual_160
    A, b, c, lo, hi, basis, up = L.at(cs)
    mx = cs["maximize"]
    j = int(np.flatnonzero(np.isfinite(hi) & (np.asarray(up) == 0))[0])
    crossed, rep = _changed(hi, j, lo[j] - 0.25), _changed(basis, 3, basis[0])
    A1, b1, c1, lo1, hi1, _ = Q.singular(1)   # rows 0 and m-1 of A are equal, so is every basis of original columns
    cases = [((A, b, c, lo, crossed, basis, up), INFEASIBLE),
             ((A, b, c, lo, hi, rep, up), SINGULAR),
             ((A1, b1, c1, lo1, hi1, basis, up), None),       # whatever the reference says
             ((A, b, c, lo, crossed, rep, up), None),
             ((A1, b1, c1, lo1, crossed, basis, up), None)]
    for bad, status in cases:
        want = CR.certificate(*bad, mx)
        assert want["status"] != OPTIMAL and (status is None or want["status"] == status)
        got = ctx.basis_bounded_certificate_large(*bad, mx)
        _same(got, want)
        assert got["kind"] == L.NONE and got["index"] == -1 and np.isnan(got["value"])
        assert np.isnan(got["farkas"]).all() and np.isnan(got["ray"]).all()
        _good_call(ctx, dual_160)


def test_refusals_at_160x320(ctx, dual_160):
    cs, _ = dual_160
    A, b, c, lo, hi, basis, up = L.at(cs)
    mx = cs["maximize"]
    m, n = A.shape
    free = int(np.flatnonzero(np.isinf(hi))[0])
    refusals = [dict(lo=_changed(lo, 0, np.nan)), dict(lo=_changed(lo, 0, -np.inf)), dict(lo=_changed(lo, 0, np.inf)),
                dict(hi=_changed(hi, 0, np.nan)),
                dict(up=_changed(up, 0, 2)), dict(up=_changed(np.zeros(n, np.int32), free, 1)),
                dict(basis=_changed(basis, 1, n + m)), dict(basis=_changed(basis, 1, -1))]
    for kw in refusals:
        args = dict(lo=lo, hi=hi, basis=basis, up=up)
        args.update(kw)
        bad = (A, b, c, args["lo"], args["hi"], args["basis"], args["up"])
        assert CR.certificate(*bad, mx)["status"] == BAD_ARG
        with pytest.raises(capi.LPError) as e:
            ctx.basis_bounded_certificate_large(*bad, mx)
        assert e.value.code == BAD_ARG, kw
    for eps in (-1e-12, float("nan")):
        assert CR.certificate(*L.at(cs), mx, eps)["status"] == BAD_ARG
        with pytest.raises(capi.LPError) as e:
            ctx.basis_bounded_certificate_large(*L.at(cs), mx, eps)
        assert e.value.code == BAD_ARG
    _good_call(ctx, dual_160)


def test_null_pointers_are_refused(ctx, dual_160):
    cs, want = dual_160
    A, b, c, lo, hi, basis, up = L.at(cs)
    m, n = A.shape
    basis, up = np.ascontiguousarray(basis, np.int32), np.ascontiguousarray(up, np.int32)
    Af = capi.colmajor(A)
    kind, index = np.zeros(1, np.int32), np.zeros(1, np.int32)
    farkas, ray, value = np.zeros(m), np.zeros(n), np.zeros(1)
    dp, ip = capi._d, capi._i
    f = [np.ascontiguousarray(v, np.float64) for v in (b, c, lo, hi)]
    args = [ctx.h, dp(Af), m, n, dp(f[0]), dp(f[1]), dp(f[2]), dp(f[3]), ip(basis), ip(up), int(cs["maximize"]), 1e-9,
            ip(kind), dp(farkas), dp(ray), dp(value), ip(index)]
    fn = ctx.lib.lp_basis_bounded_certificate_large
    for k in (1, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16):
        bad = list(args)
        bad[k] = None
        assert fn(*bad) == BAD_ARG, k
    assert fn(*args) == OPTIMAL   # the full call is good, and the context still is
    got = dict(status=OPTIMAL, kind=int(kind[0]), farkas=farkas, ray=ray, value=float(value[0]), index=int(index[0]))
    _same(got, want)
