"""Farkas and unbounded-ray certificates of bounded-variable LPs on the GPU (lp_basis_bounded_certificate and its batched
form): every output equals tests/ref/bounded_certificate_ref.c's bit for bit (NaN where it has NaN, signed zeros
included) at the bases and flags the GPU's own bounded solves and re-solves stopped at, on shapes that reach every path
of the kernel, with and without run statuses; the GPU's vectors pass the numpy checks of the CPU tests; eps = 0 and
1e-12; the per-LP statuses; the whole-call refusals; the anchor on lp_basis_certificate_batched; and the chain after
lp_mip_bounded_solve_batched."""
import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import bounded_certcases as BC
from tests import bounded_certificate_ref as R
from tests import bounded_ref as B
from tests import bounded_resolve_ref as BR
from tests import certcases as CC
from tests import mip_bounded_ref as MB

pytestmark = pytest.mark.gpu

NONE, FARKAS, RAY = R.NONE, R.FARKAS, R.RAY
FAMILIES = ("infeasible", "unbounded", "rich", "mixed", "dual")


def _row(out, k):
    return {key: v[k] for key, v in out.items()}


def gpu_mix(ctx, m, n, maximize, per_family=4):
    """A batch mixing all families at one shape and sense, solved on the GPU: the cold LPs by bounded_batched, the "dual"
    ones then re-solved by bounded_resolve_batched under tightened bounds (seeds the CPU reference drives to INFEASIBLE
    first, then others).  Returns (at, run, names): at = (A, b, c, lo, hi, basis, at_upper) of the final LPs."""
    dual = [s for s in range(40) if BC.dual_infeasible(s, m, n, maximize=maximize) is not None][:per_family - 1]
    dual += [s for s in range(40) if s not in dual][:per_family - len(dual)]
    lps, names = [], []
    for fam in FAMILIES:
        for q in range(per_family):
            if fam == "rich":
                lp = BC.rich_unbounded_lp(q, m, n, maximize)
            elif fam == "dual":
                lp = B.boxed_lp(dual[q], m, n, maximize, kind="mixed")
            else:
                lp = B.boxed_lp(q, m, n, maximize, kind=fam)
            lps.append(lp[:5])
            names.append(fam)
    A, b, c, lo, hi = (np.stack([lp[i] for lp in lps]) for i in range(5))
    cold = ctx.bounded_batched(A, b, c, lo, hi, maximize)
    basis, up, run = cold["basis"].copy(), cold["at_upper"].copy(), cold["status"].copy()
    sel = [k for k, fam in enumerate(names) if fam == "dual" and run[k] == R.OPTIMAL]
    for k in sel:
        seed = dual[k - names.index("dual")]
        _, _, lo[k], hi[k] = BR.perturb(seed, "bound", b[k], c[k], lo[k], hi[k], basis[k], cold["x"][k])
    warm = ctx.bounded_resolve_batched(A[sel], b[sel], c[sel], lo[sel], hi[sel], basis[sel], up[sel], maximize)
    basis[sel], up[sel], run[sel] = warm["basis"], warm["at_upper"], warm["status"]
    return (A, b, c, lo, hi, basis, up), run, names


# (13, 40): m no multiple of the 8-row tile; (40, 300): a second 256-column chunk; (72, 150): 512 threads, the crash
# rows written by waves other than wave 0
@pytest.mark.parametrize("m,n", [(4, 12), (13, 40), (32, 96), (40, 300), (72, 150)])
@pytest.mark.parametrize("maximize", [True, False])
def test_single_and_batched_at_the_gpus_own_bases(ctx, m, n, maximize):
    assert ctx.basis_bounded_certificate_fits(m, n)
    at, run, names = gpu_mix(ctx, m, n, maximize)
    batch = len(names)
    assert 12 <= batch <= 24
    for fam, st in zip(names, run):
        want = {"infeasible": R.INFEASIBLE, "unbounded": R.UNBOUNDED, "rich": R.UNBOUNDED}.get(fam)
        assert want is None or st == want, (fam, st)
    # with the run statuses: only the failed LPs are analysed
    want = R.certificate_batched(*at, maximize, run_status=run)
    got = ctx.basis_bounded_certificate_batched(*at, maximize, run_status=run)
    R.same_bits(got, want)
    assert np.array_equal(got["status"], run)
    for k, fam in enumerate(names):
        if fam == "infeasible":
            assert got["kind"][k] == FARKAS and got["index"][k] == -1
        elif fam in ("unbounded", "rich"):
            assert got["kind"][k] == RAY
            assert fam == "unbounded" or np.count_nonzero(got["ray"][k]) > 1
        elif run[k] == R.OPTIMAL:
            assert got["kind"][k] == NONE
        elif run[k] == R.INFEASIBLE and not np.any(at[4][k] < at[3][k]):
            assert got["kind"][k] == FARKAS and (fam != "dual" or got["index"][k] >= 0)
    assert any(fam == "dual" and got["kind"][k] == FARKAS and got["index"][k] >= 0 for k, fam in enumerate(names))
    # without: every LP gets its case analysis, and the batch is the single call per LP
    want = R.certificate_batched(*at, maximize)
    got = ctx.basis_bounded_certificate_batched(*at, maximize)
    R.same_bits(got, want)
    for k in range(batch):
        one = ctx.basis_bounded_certificate(*(v[k] for v in at), maximize)
        R.same_bits(one, _row(got, k))
        if got["status"][k] == R.OPTIMAL:
            BC.check(dict(A=at[0][k], b=at[1][k], c=at[2][k], lo=at[3][k], hi=at[4][k], maximize=maximize), one)
            if run[k] == R.OPTIMAL:
                assert one["kind"] == NONE


@pytest.mark.parametrize("eps", [0.0, 1e-12])
def test_eps_on_an_infeasible_batch(ctx, eps):
    m, n = 12, 32
    cases = [BC.cold(s, m, n, "infeasible", solve=ctx.bounded, maximize=True) for s in range(6)]
    cases += [cs for cs in (BC.dual_infeasible(s, m, n, resolve=ctx.bounded_resolve, maximize=True) for s in range(40))
              if cs is not None][:6]
    assert len(cases) == 12 and all(cs["run"] == R.INFEASIBLE for cs in cases)
    s = BC.stack(cases)
    at = tuple(s[k] for k in ("A", "b", "c", "lo", "hi", "basis", "at_upper"))
    want = R.certificate_batched(*at, True, eps)
    got = ctx.basis_bounded_certificate_batched(*at, True, eps)
    R.same_bits(got, want)
    assert (got["status"] == R.OPTIMAL).all()
    for k, cs in enumerate(cases):
        BC.check(cs, _row(got, k))


def test_statuses_in_one_batch(ctx):
    m, n = 6, 16
    cs = BC.cold(1, m, n, "infeasible", solve=ctx.bounded, maximize=True)
    at = [np.stack([cs[k]] * 4) for k in ("A", "b", "c", "lo", "hi", "basis", "at_upper")]
    A, lo, hi, basis, up = at[0], at[3], at[4], at[5], at[6]
    basis[0] = np.arange(m)
    basis[0, 2] = basis[0, 0]                   # LP 0: a repeated index
    basis[1] = np.arange(m)
    up[0] = up[1] = 0
    hi[0] = hi[1] = np.inf
    A[1][:, 1] = 2.0 * A[1][:, 0]               # LP 1: dependent basic columns
    hi[2, 3] = lo[2, 3] - 0.5                   # LP 2: crossed bounds; LP 3 is fine
    want = R.certificate_batched(*at, True)
    assert want["status"].tolist() == [R.SINGULAR, R.SINGULAR, R.INFEASIBLE, R.OPTIMAL] and want["kind"][3] == FARKAS
    got = ctx.basis_bounded_certificate_batched(*at, True)
    R.same_bits(got, want)
    for k in range(4):
        R.same_bits(ctx.basis_bounded_certificate(*(v[k] for v in at), True), _row(want, k))
    # under run statuses the own failure still shows, and an LP that did not fail is left alone
    run = np.array([R.INFEASIBLE, R.OPTIMAL, R.INFEASIBLE, R.INFEASIBLE], np.int32)
    want = R.certificate_batched(*at, True, run_status=run)
    assert want["status"].tolist() == [R.SINGULAR, R.OPTIMAL, R.INFEASIBLE, R.INFEASIBLE]
    R.same_bits(ctx.basis_bounded_certificate_batched(*at, True, run_status=run), want)


def test_whole_call_refusals_then_a_good_call(ctx):
    m, n = 8, 20
    cs = BC.cold(0, m, n, "infeasible", solve=ctx.bounded, maximize=True)
    A, b, c, lo, hi, basis, up = (cs[k] for k in ("A", "b", "c", "lo", "hi", "basis", "at_upper"))
    free = int(np.flatnonzero(np.isinf(hi))[0])

    def changed(v, at, val):
        v = v.copy()
        v[at] = val
        return v

    refusals = [dict(basis=changed(basis, 1, n + m)), dict(basis=changed(basis, 1, -1)),
                dict(up=changed(np.zeros(n, np.int32), free, 1)), dict(up=changed(up, 0, 2)),
                dict(hi=changed(hi, 0, np.nan)), dict(lo=changed(lo, 0, -np.inf)), dict(eps=-1.0),
                dict(eps=float("nan"))]
    for kw in refusals:
        args = dict(lo=lo, hi=hi, basis=basis, up=up, eps=1e-9)
        args.update(kw)
        at = (A, b, c, args["lo"], args["hi"], args["basis"], args["up"])
        two = [np.stack([v, v]) for v in (A, b, c, lo, hi, basis, up)]
        for i, v in enumerate(at):
            two[i][1] = v   # only the second LP is bad
        for call in (lambda: ctx.basis_bounded_certificate(*at, True, args["eps"]),
                     lambda: ctx.basis_bounded_certificate_batched(*two, True, args["eps"]),
                     lambda: ctx.basis_bounded_certificate_batched(*two, True, args["eps"],
                                                                   run_status=np.array([4, 0], np.int32))):
            with pytest.raises(capi.LPError) as e:
                call()
            assert e.value.code == R.BAD_ARG, kw
    big = B.boxed_lp(0, 160, 320)   # beyond lp_basis_bounded_certificate_fits
    assert not ctx.basis_bounded_certificate_fits(160, 320)
    with pytest.raises(capi.LPError) as e:
        ctx.basis_bounded_certificate(*big[:5], np.arange(320, 480, dtype=np.int32), np.zeros(320, np.int32))
    assert e.value.code == R.BAD_ARG
    at = (A, b, c, lo, hi, basis, up)
    good = ctx.basis_bounded_certificate(*at, True)
    R.same_bits(good, R.certificate(*at, True))
    assert good["kind"] == FARKAS


def test_without_bounds_it_is_the_unbounded_certificate(ctx):
    m, k = 10, 16
    A, b, c, _ = CC.two_phase_mix(100 * m, 16, m, k)
    n = k + m
    basis = np.stack([o.two_phase(A[q], b[q], c[q], False)["basis"] for q in range(len(A))]).astype(np.int32)
    lo, hi, up = np.zeros((len(A), n)), np.full((len(A), n), np.inf), np.zeros((len(A), n), np.int32)
    got = ctx.basis_bounded_certificate_batched(A, b, c, lo, hi, basis, up, False)
    want = ctx.basis_certificate_batched(A, b, c, basis, False)
    R.same_bits(got, want)
    assert set(got["kind"].tolist()) == {NONE, FARKAS, RAY}


def test_after_the_bounded_branch_and_bound(ctx):
    """The statuses of lp_mip_bounded_solve_batched chain: a problem whose root is infeasible gets its FARKAS from the
    root basis, a solved one keeps its status and gets NONE."""
    m, n = 5, 14
    ps = [MB.boxed_mip(s, m, n, True, kind="infeasible" if s % 2 else "mixed", every=2) for s in range(6)]
    A, b, c, lo, hi = (np.stack([p[i] for p in ps]) for i in range(5))
    mask = ps[0][5]
    cold = ctx.bounded_batched(A, b, c, lo, hi, True)
    ok = cold["status"] == R.OPTIMAL
    assert (cold["status"][1::2] == R.INFEASIBLE).all() and ok[0::2].any()
    mip = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, np.where(ok[:, None], cold["basis"], 0),
                                        np.where(ok[:, None], cold["at_upper"], 0), cold["status"], True)
    assert np.array_equal(mip["status"][1::2], cold["status"][1::2])
    at = (A, b, c, lo, hi, cold["basis"], cold["at_upper"])
    got = ctx.basis_bounded_certificate_batched(*at, True, run_status=mip["status"])
    R.same_bits(got, R.certificate_batched(*at, True, run_status=mip["status"]))
    assert np.array_equal(got["status"], mip["status"])
    for k in range(len(ps)):
        if k % 2:
            assert got["kind"][k] == FARKAS and got["index"][k] == -1
            BC.check(dict(A=A[k], b=b[k], c=c[k], lo=lo[k], hi=hi[k], maximize=True), _row(got, k))
        elif mip["status"][k] == R.OPTIMAL:
            assert got["kind"][k] == NONE
