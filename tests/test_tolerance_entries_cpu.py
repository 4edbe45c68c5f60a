"""The inputs of tests/tolentries.py on the CPU references alone (no GPU): they must depend on eps, or the GPU parity
tests of tests/test_gpu_tolerance_entries.py would pass without looking at anything.  Conditions, not measurements;
a seed of tolentries.py that misses one is replaced by the first of 0..31 that meets it, the condition stays.

  A  Devex: at each shape the reference at eps = 0 differs from the one at 1e-9 on at least 3 of the 7 LPs, from the
     slack basis (trace) and in the two-phase form (the three pivot counts); the two cost scalings by 2^+-600 change
     the number of pivots at eps = 0 (the squared scores d * d / w leave fp64), those by 2^+-300 do not.
  B  Bounded re-solve: at each eps of the grid at most 2 of the 7 cold solves are not OPTIMAL; at each shape at least
     2 LPs differ in status or counters between eps = 0 and 1e-9 under the "bound" perturbation; at each shape and
     eps at least one "cost" perturbation ends with a bound flip.
  C  Bounded MIP: at each shape at least 3 LPs of the batch have other stats at 1e-2 than at 1e-9, at least 3 of the
     exact-tie LPs have another status or other stats at eps = 0 than at 1e-9, and at eps = 0 at least 2 LPs are
     searched beyond their root.
  D  Parametric RHS and cost: at each eps at least 3 of the 7 LPs have nseg >= 2; at each shape at least 2 LPs have
     another nseg at eps = 0 than at 1e-9.

-0.0 is +0.0 for every reference, bit for bit."""
import numpy as np
import pytest

from tests import devex_ref as D
from tests import tolentries as E

SHAPE_IDS = [f"{m}x{n}" for m, n in E.SHAPES]
BATCH = len(E.PICKS)


def _bits(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return v[~np.isnan(v)].view(np.uint64).tolist(), np.isnan(v).tolist()


# ---- A ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", E.SHAPES, ids=SHAPE_IDS)
def test_devex_depends_on_eps(m, n):
    A, b, c, basis = E.mixed(m, n)
    A2, b2, c2 = E.two_phase_form(A, b, c)
    slack = two_phase = 0
    for k in range(BATCH):
        r0, r9 = (D.simplex_tableau(A[k], b[k], c[k], basis[k], True, n - m, eps=e, trace_cap=1 << 14)
                  for e in (0.0, E.EPS_DEFAULT))
        slack += r0["trace"] != r9["trace"]
        t0, t9 = (D.two_phase(A2[k], b2[k], c2[k], True, n - m, eps=e) for e in (0.0, E.EPS_DEFAULT))
        two_phase += t0["iters"] != t9["iters"]
    assert slack >= 3 and two_phase >= 3, (slack, two_phase)


@pytest.mark.parametrize("fam,seed,idx", E.SCALED, ids=[s[0] for s in E.SCALED])
def test_devex_scaled_costs_change_the_path_only_past_fp64(fam, seed, idx):
    def pivots(k):
        A, b, c, basis = E.scaled_cost_case(fam, seed, idx, k)
        r = D.simplex_tableau(A, b, c, basis, True, A.shape[1] - A.shape[0], eps=0.0)
        assert r["status"] == E.OPTIMAL
        return r["iters"]
    plain = pivots(0)
    assert plain > 0
    for k in E.SCALED_DIFFERENT:
        assert pivots(k) != plain, k
    for k in E.SCALED_SAME:
        assert pivots(k) == plain, k


# ---- B ---------------------------------------------------------------------------------------------------------------
def _resolve_outcomes(m, n, eps, kind):
    keep, _ = E.resolve_batch(m, n, eps, kind)
    return {k: (r["status"], tuple(r["iters"])) for k, r in zip(keep, E.resolve_ref(m, n, eps, kind))}


@pytest.mark.parametrize("m,n", E.SHAPES, ids=SHAPE_IDS)
def test_bounded_resolve_depends_on_eps(m, n):
    for eps in E.EPS:
        cold = E.same_eps_start("bounded", m, n, eps)
        assert sum(r["status"] != E.OPTIMAL for r in cold) <= 2, eps
        flips = [it[2] for _, it in _resolve_outcomes(m, n, eps, "cost").values()]
        assert max(flips) > 0, eps
    r0, r9 = (_resolve_outcomes(m, n, e, "bound") for e in (0.0, E.EPS_DEFAULT))
    assert sum(r0.get(k) != r9.get(k) for k in range(BATCH)) >= 2
    assert any(it[0] > 0 for _, it in r0.values())   # the dual loop runs at eps = 0


def test_bounded_resolve_has_no_cold_start_at_inf():
    """Why the entry is run at +inf from the start of the default eps (tolentries.start_eps)."""
    from tests import bounded_ref
    A, b, c, lo, hi = E.bounded_lps(*E.SMALL)
    for k in range(BATCH):
        assert bounded_ref.bounded(A[k], b[k], c[k], lo[k], hi[k], True, eps=np.inf)["status"] != E.OPTIMAL


# ---- C ---------------------------------------------------------------------------------------------------------------
def _mip_outcomes(m, n, eps):
    return [(root["status"], None if r is None else (r["status"], r["found"], r["stats"]))
            for root, r in E.mip_ref(m, n, eps)]


@pytest.mark.parametrize("m,n", E.SHAPES, ids=SHAPE_IDS)
def test_bounded_mip_depends_on_eps(m, n):
    r0, r9, r2 = (_mip_outcomes(m, n, e) for e in (0.0, E.EPS_DEFAULT, 1e-2))
    assert all(root == E.OPTIMAL for root, _ in r9)
    assert sum(a != b for a, b in zip(r2, r9)) >= 3
    assert sum(a != b for a, b in zip(r0[:E.MIP_TIES], r9[:E.MIP_TIES])) >= 3
    searched = [r for _, r in r0 if r is not None and r[0] != 5 and r[2][0] > 1]
    assert len(searched) >= 2
    assert sum(r[2][0] > 1 for _, r in r9) >= 5   # the tie family branches (b + 0.5)


# ---- D ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rhs", "cost"])
@pytest.mark.parametrize("m,n", E.SHAPES, ids=SHAPE_IDS)
def test_parametric_depends_on_eps(m, n, which):
    for eps in E.EPS:
        cold = E.same_eps_start("oracle", m, n, eps, E.PARAMETRIC_SEED[(m, n)])
        assert all(r["status"] == E.OPTIMAL for r in cold), eps
        assert (E.parametric_refs(m, n, eps, which)["nseg"] >= 2).sum() >= 3, eps
    n0, n9 = (E.parametric_refs(m, n, e, which)["nseg"] for e in (0.0, E.EPS_DEFAULT))
    assert (n0 != n9).sum() >= 2


def test_a_basis_of_the_default_eps_is_refused_at_eps_zero():
    """Why the start of a composite entry is solved at the entry's own eps."""
    from tests import parametric_ref as P
    m, n = E.LARGE
    A, b, c, basis9, d, _, _ = E.parametric_inputs(m, n, E.EPS_DEFAULT)
    ok9 = [P.parametric(A[k], b[k], c[k], basis9[k], d[k], eps=E.EPS_DEFAULT)["status"] != P.BAD_ARG
           for k in range(BATCH)]
    bad0 = [P.parametric(A[k], b[k], c[k], basis9[k], d[k], eps=0.0)["status"] == P.BAD_ARG for k in range(BATCH)]
    assert sum(a and r for a, r in zip(ok9, bad0)) >= 3


# ---- -0.0 ------------------------------------------------------------------------------------------------------------
def test_negative_zero_is_zero_for_every_reference():
    m, n = E.SMALL
    for which in ("rhs", "cost"):
        a, z = (E.parametric_refs(m, n, e, which) for e in (-0.0, 0.0))
        for key in a:
            assert _bits(a[key]) == _bits(z[key]), (which, key)
    for kind in ("bound", "rhs", "cost"):
        for a, z in zip(E.resolve_ref(m, n, -0.0, kind), E.resolve_ref(m, n, 0.0, kind)):
            assert a["status"] == z["status"] and a["iters"] == z["iters"] and _bits(a["x"]) == _bits(z["x"])
    assert _mip_outcomes(m, n, -0.0) == _mip_outcomes(m, n, 0.0)


def test_inputs_are_deterministic():
    m, n = E.SMALL
    for make in (lambda: E.boxed_mip_ties(m, n, 3), lambda: E.bounded_lps(m, n), lambda: E.mixed(m, n)):
        a = make()
        E._CACHE.clear()
        for x, y in zip(a, make()):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
