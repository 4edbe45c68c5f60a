"""Farkas and unbounded-ray certificates on the GPU (lp_basis_certificate, lp_basis_certificate_batched,
lp_batched_certificates): kind, index, status and every value bit for bit against tests/ref/certificate_ref.c, NaNs
included, on both sides of lp_basis_certificate_fits, after plain and two-phase batch runs under both pivot rules
and after a re-solve run, on the per-LP fallback, and at the final bases of the single-LP solvers.  On top of that
the GPU's own vectors are checked with numpy, and every infeasible or unbounded family gets a certificate."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import certcases as CC
from tests import certificate_ref as R
from tests.test_certificate_cpu import check

pytestmark = pytest.mark.gpu

OPTIMAL_FAMILIES = {"optimal"}


def _bits(a):
    a = np.asarray(a, dtype=np.float64)
    return np.isnan(a), a.view(np.uint64)


def _same(g, r):
    """Bit for bit, NaN where the reference has NaN (signed zeros included)."""
    for key in ("status", "kind", "index"):
        assert np.array_equal(np.asarray(g[key]), np.asarray(r[key])), key
    for key in ("farkas", "ray", "value"):
        ng, bg = _bits(g[key])
        nr, br = _bits(r[key])
        assert np.array_equal(ng, nr), key
        assert np.array_equal(bg[~ng], br[~nr]), key


def _check_batch(A, b, c, maximize, g, names):
    """numpy properties of each GPU certificate; a family without an optimum must get one."""
    for q, fam in enumerate(names):
        one = {key: (g[key][q] if np.ndim(g[key]) else g[key]) for key in g}
        if one["status"] in (capi.INFEASIBLE, capi.UNBOUNDED):
            one = dict(one, status=0)
        check(A[q], b[q], c[q], maximize, one)
        if fam not in OPTIMAL_FAMILIES:
            want = capi.CERT_RAY if "unbounded" in fam else capi.CERT_FARKAS
            assert g["kind"][q] == want, (q, fam)
        else:
            assert g["kind"][q] == capi.CERT_NONE


@pytest.mark.parametrize("rule", ["dantzig", "bland"])
@pytest.mark.parametrize("m,k", [(12, 20), (64, 128), (96, 96)])   # 256 and 512 threads per workgroup
def test_two_phase_batch(ctx, rule, m, k):
    A, b, c, names = CC.two_phase_mix(300 + m, 24, m, k)
    assert ctx.basis_certificate_fits(m, k + m)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False)
    try:
        assert p.path() == 1
        p.set_pivot_rule(rule)
        p.run()
        s = p.download()
        g = p.certificates()
    finally:
        p.free()
    for q, fam in enumerate(names):
        assert s["status"][q] == {"optimal": 0, "phase2_unbounded": 1}.get(fam, 4), (q, fam)
    _same(g, R.certificate_batched(A, b, c, s["basis"], False, run_status=s["status"]))
    _check_batch(A, b, c, False, g, names)


@pytest.mark.parametrize("rule", ["dantzig", "bland"])
@pytest.mark.parametrize("m,n", [(16, 40), (128, 256)])
def test_plain_batch(ctx, rule, m, n):
    A, b, c, basis, names = CC.plain_mix(700 + m, 12, m, n)
    p = ctx.batched_problem(A, b, c, basis, True)
    try:
        assert p.path() == 1
        p.set_pivot_rule(rule)
        p.run()
        s = p.download()
        g = p.certificates()
    finally:
        p.free()
    assert [int(v) for v in s["status"]] == [0 if f == "optimal" else 1 for f in names]
    _same(g, R.certificate_batched(A, b, c, s["basis"], True, run_status=s["status"]))
    _check_batch(A, b, c, True, g, names)
    # every LP at its final basis, whatever its run status: the batched call without run statuses
    h = ctx.basis_certificate_batched(A, b, c, s["basis"], True)
    _same(h, R.certificate_batched(A, b, c, s["basis"], True))


@pytest.mark.parametrize("m,n", [(32, 96), (96, 192)])   # 256 and 512 threads per workgroup
def test_resolve_batch(ctx, m, n):
    """The re-solve handle runs Dantzig's rule only (Bland's is LP_BAD_ARG there).  96 x 192 is close to the
    largest re-solve shape with 96 rows (lp_batched_two_phase_fits); its dual-simplex certificates take rows of
    B^-1 that waves other than wave 0 write."""
    assert ctx.basis_certificate_fits(m, n)
    A, b, b2, c, basis, names = CC.resolve_mix(900 + m, 16, m, n)
    cold = ctx.simplex_solve_batched(A, b, c, basis, True)
    assert (cold["status"] == capi.OPTIMAL).all()
    p = ctx.batched_resolve_problem(A, b2, c, cold["basis"], True)
    try:
        assert p.path() == 1
        p.run()
        s = p.download()
        g = p.certificates()
        g0 = p.certificates(eps=0.0)
    finally:
        p.free()
    assert [int(v) for v in s["status"]] == [0 if f == "optimal" else 4 for f in names]
    _same(g, R.certificate_batched(A, b2, c, s["basis"], True, run_status=s["status"]))
    _same(g0, R.certificate_batched(A, b2, c, s["basis"], True, eps=0.0, run_status=s["status"]))
    _check_batch(A, b2, c, True, g, names)


def test_fallback_handle(ctx):
    """A plain handle whose starting bases are not the slack identity runs the per-LP fallback."""
    m, n = 16, 40
    A, b, c, basis, names = CC.plain_mix(40, 6, m, n)
    basis = basis[:, ::-1].copy()   # the slack basis, positions reversed
    p = ctx.batched_problem(A, b, c, basis, True)
    try:
        assert p.path() == 0
        p.run()
        s = p.download()
        g = p.certificates()
    finally:
        p.free()
    assert [int(v) for v in s["status"]] == [0 if f == "optimal" else 1 for f in names]
    _same(g, R.certificate_batched(A, b, c, s["basis"], True, run_status=s["status"]))
    _check_batch(A, b, c, True, g, names)


@pytest.mark.parametrize("m,n", [(40, 100), (128, 256), (160, 320)])
@pytest.mark.parametrize("algo", [capi.SIMPLEX_AUTO, capi.SIMPLEX_LAUNCH])
def test_single_lp_both_sides_of_fits(ctx, m, n, algo):
    assert ctx.basis_certificate_fits(m, n) == (m <= 128)
    for fam, gen in (("unbounded_obvious", CC.unbounded_obvious), ("unbounded_after_pivots", CC.unbounded_after_pivots),
                     ("optimal", capi.gen_lp)):
        A, b, c, basis = gen(11 * m, m, n)
        p = ctx.simplex_problem(A, b, c, basis, True)
        try:
            rc, _ = p.run(algo=algo)
            fb = p.download()["basis"]
        finally:
            p.free()
        assert rc == (capi.OPTIMAL if fam == "optimal" else capi.UNBOUNDED)
        g = ctx.basis_certificate(A, b, c, fb, True)
        r = R.certificate(A, b, c, fb, True)
        _same(g, r)
        check(A, b, c, True, g)
        assert g["kind"] == (capi.CERT_NONE if fam == "optimal" else capi.CERT_RAY)
        h = ctx.basis_certificate_batched(A[None], b[None], c[None], fb[None], True)   # batch of one
        _same({k: v[0] for k, v in h.items()}, r)


@pytest.mark.parametrize("m,k", [(12, 20), (140, 150)])
def test_single_two_phase(ctx, m, k):
    """lp_simplex_two_phase's final bases (phase-I bases with artificials when infeasible), beyond fits too."""
    A, b, c, names = CC.two_phase_mix(50 + m, 4, m, k)
    assert ctx.basis_certificate_fits(m, k + m) == (m <= 132)
    for q, fam in enumerate(names):
        s = ctx.two_phase(A[q], b[q], c[q], False)
        assert s["status"] == {"optimal": 0, "phase2_unbounded": 1}.get(fam, 4), fam
        g = ctx.basis_certificate(A[q], b[q], c[q], s["basis"], False)
        _same(g, R.certificate(A[q], b[q], c[q], s["basis"], False))
        check(A[q], b[q], c[q], False, g)
        want = {"optimal": capi.CERT_NONE, "phase2_unbounded": capi.CERT_RAY}.get(fam, capi.CERT_FARKAS)
        assert g["kind"] == want, fam


def test_dual_simplex_beyond_fits(ctx):
    """The dual-simplex case on the single-LP path beyond fits: a re-solve that ends infeasible."""
    m, n = 160, 320
    A, b, b2, c, basis, names = CC.resolve_mix(77, 2, m, n)
    q = names.index("infeasible_after_resolve")
    cold = ctx.simplex_solve(A[q], b[q], c[q], basis[q], True)
    s = ctx.simplex_resolve(A[q], b2[q], c[q], cold["basis"], True)
    assert s["status"] == capi.INFEASIBLE
    g = ctx.basis_certificate(A[q], b2[q], c[q], s["basis"], True)
    _same(g, R.certificate(A[q], b2[q], c[q], s["basis"], True))
    assert g["kind"] == capi.CERT_FARKAS and g["index"] >= 0
    check(A[q], b2[q], c[q], True, g)


@pytest.mark.parametrize("m,n", [(8, 20), (150, 300)])
def test_statuses(ctx, m, n):
    A, b, c, basis = capi.gen_lp(5, m, n)
    with pytest.raises(capi.LPError) as e:
        ctx.basis_certificate(A, b, c, np.r_[basis[:-1], n + m])
    assert e.value.code == capi.BAD_ARG
    with pytest.raises(capi.LPError):
        ctx.basis_certificate(A, b, c, basis, eps=-1.0)
    rep = basis.copy()
    rep[1] = rep[0]
    g = ctx.basis_certificate(A, b, c, rep)
    assert g["status"] == capi.SINGULAR and g["kind"] == capi.CERT_NONE and np.isnan(g["farkas"]).all()
    A2 = A.copy()
    A2[:, basis[1]] = 2.0 * A2[:, basis[0]]
    g = ctx.basis_certificate(A2, b, c, basis)
    _same(g, R.certificate(A2, b, c, basis))
    assert g["status"] == capi.SINGULAR
    # per-LP statuses of a batch: out of range, repeated, singular, fine
    bases = np.stack([np.r_[basis[:-1], n + m], rep, basis, basis])
    As = np.stack([A, A, A2, A])
    h = ctx.basis_certificate_batched(As, np.stack([b] * 4), np.stack([c] * 4), bases)
    assert list(h["status"]) == [capi.BAD_ARG, capi.SINGULAR, capi.SINGULAR, capi.OPTIMAL]
    _same(h, R.certificate_batched(As, np.stack([b] * 4), np.stack([c] * 4), bases))
