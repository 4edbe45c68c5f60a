"""The basis analyses at exact ties and eps edges (tests/tiecases.py; its conditions are asserted without a GPU in
tests/test_basis_ties_cpu.py): duals, RHS / cost ranging and the Farkas / ray certificates, plain and bounded, as one LP
per workgroup, batched, and on the tableau in HBM.  Every output field equals the C reference's bit for bit (floats by
their uint64 view, so NaN where it has NaN and signed zeros included; indices, sides, kind and status), in both senses
and over the eps grid, and where a shape runs on two paths the two results are equal.

Left out: the handle forms (BatchedProblem.ranging and .certificates after a run).  A run ends at the designed basis
only if that basis is optimal for the solver's own pivoting, which the designed reduced costs are not meant to be."""
import numpy as np
import pytest

from tests import bounded_certificate_ref as BC
from tests import bounded_sens_ref as S
from tests import certificate_ref as PC
from tests import duals_ref as PD
from tests import ranging_ref as PR
from tests import tiecases as T

pytestmark = pytest.mark.gpu

OPTIMAL, SINGULAR = 0, 3
PLAIN_RANGING = ("b_lo", "b_hi", "b_leave", "c_lo", "c_hi", "c_enter")
PLAIN_DUALS = ("y", "d", "w")
SENSES = (False, True)

_cache = {}


def ref(key, fn, *args):
    """fn(*args), computed once per key and left unchanged."""
    if key not in _cache:
        _cache[key] = fn(*args)
    return _cache[key]


def _same(got, want, keys):
    assert np.array_equal(np.asarray(got["status"]), np.asarray(want["status"]))
    S.same_bits(got, want, keys)


def _fits_bounded(ctx, m, n):
    return ctx.basis_bounded_fits(m, n)


# ------------------------------------------------------------------------------------------- ranging and duals, single
@pytest.mark.parametrize("form,seed,m,n", T.RANGING)
def test_duals(ctx, form, seed, m, n):
    at = T.ranging_ties(form, seed, m, n)
    if form == "plain":
        want = ref(("d", form, seed, m, n), PD.duals, *at)
        assert want["status"] == OPTIMAL
        _same(ctx.basis_duals(*at), want, PLAIN_DUALS)
        large = ctx.bounded_duals_large(*T.as_bounded(at))   # without bounds: the plain analysis on the other path
        _same(large, want, ("y", "d"))
        assert S.bits(large["w"]) == S.bits(want["w"])
        return
    want = ref(("d", form, seed, m, n), S.duals, *at)
    assert want["status"] == OPTIMAL
    _same(ctx.bounded_duals_large(*at), want, S.DUALS_KEYS)
    assert _fits_bounded(ctx, m, n) == ((m, n) in T.WG_SHAPES["bounded"] + ((100, 190),))
    if _fits_bounded(ctx, m, n):
        _same(ctx.bounded_duals(*at), want, S.DUALS_KEYS)


@pytest.mark.parametrize("maximize", SENSES)
@pytest.mark.parametrize("form,seed,m,n", T.RANGING)
def test_ranging_over_the_eps_grid(ctx, form, seed, m, n, maximize):
    at = T.ranging_ties(form, seed, m, n)
    for eps in T.EPS_GRID:
        key = ("r", form, seed, m, n, maximize, eps)
        if form == "plain":
            want = ref(key, PR.ranging, *at, maximize, eps)
            assert want["status"] == OPTIMAL
            assert ctx.basis_ranging_fits(m, n) == ((m, n) in T.WG_SHAPES["plain"])
            _same(ctx.basis_ranging(*at, maximize, eps), want, PLAIN_RANGING)
            # the bounded entries without bounds: the same ends from k_bsens_* (and from k_batched_bounded_sens)
            bat = T.as_bounded(at)
            got = ctx.bounded_ranging_large(*bat, maximize, eps)
            _same(got, want, PLAIN_RANGING)
            assert set(np.unique(got["b_side"]).tolist()) <= {-1, 0}
            if _fits_bounded(ctx, m, n):
                _same(ctx.bounded_ranging(*bat, maximize, eps), got, S.RANGING_KEYS)
            continue
        want = ref(key, S.ranging, *at, maximize, eps)
        assert want["status"] == OPTIMAL
        _same(ctx.bounded_ranging_large(*at, maximize, eps), want, S.RANGING_KEYS)
        if _fits_bounded(ctx, m, n):
            _same(ctx.bounded_ranging(*at, maximize, eps), want, S.RANGING_KEYS)


# ------------------------------------------------------------------------------------------ ranging and duals, batched
def _analysis_batch(form, m, n):
    """Three seeds of ranging_ties, a dual and a ray certificate case, and a repeated basis index in the middle."""
    cases = [T.ranging_ties(form, s, m, n) for s in (1, 2)]
    cases += [T.cert_dual(form, 1, m, n)[0], T.ranging_ties(form, 3, m, n), T.cert_ray(form, 1, m, n, True)[0]]
    return T.stack(cases, 2)


@pytest.mark.parametrize("form,k", [(f, k) for f in T.FORMS for k in (0, 1)])
def test_batched_duals_and_ranging(ctx, form, k):
    m, n = T.WG_SHAPES[form][k]
    at = ref(("batch", form, m, n), _analysis_batch, form, m, n)
    if form == "plain":
        want = ref(("bd", form, m, n), PD.duals_batched, *at)
        assert want["status"].tolist() == [OPTIMAL, OPTIMAL, SINGULAR, OPTIMAL, OPTIMAL]
        _same(ctx.basis_duals_batched(*at), want, PLAIN_DUALS)
    else:
        want = ref(("bd", form, m, n), S.batched, S.duals, *at)
        assert want["status"].tolist() == [OPTIMAL, OPTIMAL, SINGULAR, OPTIMAL, OPTIMAL]
        _same(ctx.bounded_duals_batched(*at), want, S.DUALS_KEYS)
    for maximize in SENSES:
        for eps in T.EPS_GRID:
            key = ("br", form, m, n, maximize, eps)
            if form == "plain":
                _same(ctx.basis_ranging_batched(*at, maximize, eps), ref(key, PR.ranging_batched, *at, maximize, eps),
                      PLAIN_RANGING)
            else:
                _same(ctx.bounded_ranging_batched(*at, maximize, eps), ref(key, S.batched, S.ranging, *at, maximize, eps),
                      S.RANGING_KEYS)


# -------------------------------------------------------------------------------------------------------- certificates
def _cert_shapes(form):
    return T.WG_SHAPES[form] + (T.HBM_SHAPES if form == "plain" else ())


def _cert_cases(form, m, n, maximize):
    """Every cert_* family at one shape, named."""
    out = {}
    for seed in T.CERT_SEEDS:
        out["dual", seed] = T.cert_dual(form, seed, m, n)[0]
        out["ray", seed] = T.cert_ray(form, seed, m, n, maximize)[0]
        for variant in T.PHASE1_VARIANTS:
            for arts in (1, 2):
                out["phase1", variant, arts, seed] = T.cert_phase1(form, seed, m, n, variant, arts)[0]
    return out


def _certificate(ctx, form, at, maximize, eps):
    return (ctx.basis_certificate if form == "plain" else ctx.basis_bounded_certificate)(*at, maximize, eps)


def _ref_certificate(form):
    return PC.certificate if form == "plain" else BC.certificate


@pytest.mark.parametrize("maximize", SENSES)
@pytest.mark.parametrize("form,m,n", [(f, m, n) for f in T.FORMS for m, n in _cert_shapes(f)])
def test_certificates_single(ctx, form, m, n, maximize):
    """The per-workgroup kernel where the shape fits, k_cert_prepare / _columns / _finish beyond (plain only)."""
    if form == "plain":
        assert ctx.basis_certificate_fits(m, n) == ((m, n) in T.WG_SHAPES["plain"])
    else:
        assert ctx.basis_bounded_certificate_fits(m, n)
    kinds = set()
    for name, at in _cert_cases(form, m, n, maximize).items():
        for eps in T.CERT_EPS:
            want = ref(("c", form, m, n, maximize, name, eps), _ref_certificate(form), *at, maximize, eps)
            assert want["status"] == OPTIMAL
            _same(_certificate(ctx, form, at, maximize, eps), want, BC.KEYS)
            kinds.add((name[0], want["kind"]))
            if form == "plain" and ctx.basis_bounded_certificate_fits(m, n) and eps in (1e-9, 1.0):
                # without bounds the bounded kernel gives the plain certificate
                _same(ctx.basis_bounded_certificate(*T.as_bounded(at), maximize, eps), want, BC.KEYS)
    assert kinds == {("dual", BC.FARKAS), ("ray", BC.RAY), ("phase1", BC.FARKAS), ("phase1", BC.NONE)}


@pytest.mark.parametrize("maximize", SENSES)
@pytest.mark.parametrize("form,k", [(f, k) for f in T.FORMS for k in (0, 1)])
def test_certificates_batched(ctx, form, k, maximize):
    m, n = T.WG_SHAPES[form][k]
    cases = _cert_cases(form, m, n, maximize)
    names = sorted(cases, key=lambda name: (name[-1], str(name)))   # by seed, the families interleaved within it
    at = ref(("cbatch", form, m, n, maximize), T.stack, [cases[name] for name in names], len(names) // 2)
    fn = PC.certificate_batched if form == "plain" else BC.certificate_batched
    call = ctx.basis_certificate_batched if form == "plain" else ctx.basis_bounded_certificate_batched
    for eps in T.CERT_EPS:
        want = ref(("cb", form, m, n, maximize, eps), fn, *at, maximize, eps)
        assert (want["status"] == SINGULAR).sum() == 1 and want["status"][len(names) // 2] == SINGULAR
        _same(call(*at, maximize, eps), want, BC.KEYS)


# ----------------------------------------------------------------------------------------------------------- crash_tie
@pytest.mark.parametrize("p,q", T.CRASH_PAIRS_WG)
def test_crash_tie_per_workgroup(ctx, p, q):
    """ranging_crash's first maximum, in place ([B | I | b]: ranging, certificate) and on [B^T | c_B] (duals)."""
    m, n = T.CRASH_WG
    at = T.crash_tie(m, n, p, q)
    assert ctx.basis_ranging_fits(m, n) and ctx.basis_certificate_fits(m, n) and ctx.basis_duals_fits(m)
    _same(ctx.basis_duals(*at), ref(("xd", p, q), PD.duals, *at), PLAIN_DUALS)
    want = ref(("xr", p, q), PR.ranging, *at, True, 1e-9)
    assert want["status"] == OPTIMAL
    _same(ctx.basis_ranging(*at, True, 1e-9), want, PLAIN_RANGING)
    _same(ctx.basis_certificate(*at, True, 1e-9), ref(("xc", p, q), PC.certificate, *at, True, 1e-9), BC.KEYS)


def test_crash_tie_ranging_across_row_1024(ctx):
    m, n = T.CRASH_HBM
    at = T.crash_tie(m, n, *T.CRASH_PAIRS_HBM[0])
    want = ref("xr-hbm", PR.ranging, *at, True, 1e-9)
    assert want["status"] == OPTIMAL
    _same(ctx.basis_ranging(*at, True, 1e-9), want, PLAIN_RANGING)


def test_crash_tie_duals_beyond_row_1024(ctx):
    m, n = T.CRASH_HBM
    at = T.crash_tie(m, n, *T.CRASH_PAIRS_HBM[1])
    want = ref("xd-hbm", PD.duals, *at)
    assert want["status"] == OPTIMAL
    _same(ctx.basis_duals(*at), want, PLAIN_DUALS)
