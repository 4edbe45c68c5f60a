"""Bounded-variable LPs without an optimum and the numpy checks of their certificates, shared by the bounded
certificate tests and scripts/time_bounded_certificate.py (the lp_basis_bounded_certificate family).  Test
infrastructure only.

The families, each a list of dicts(A, b, c, lo, hi, maximize, basis, at_upper, run): the LP, the basis and flags a
solver reference stopped at, and its status.
- cold(kind): bounded_ref.boxed_lp(kind) solved by bounded_ref.bounded.  "infeasible" ends in phase I (artificials
  basic), "unbounded" in phase II (an all-zero column: a ray with one non-zero), "crossed" without an iteration, "mixed"
  mostly optimal.
- rich_unbounded: boxed_lp("mixed") with one structural column negated and freed to [0, inf), every slack freed to
  [0, inf) with cost 0 and the column's cost improving: the ray moves the column and the basic variables with it.
- dual_infeasible: boxed_lp("mixed") solved, one to three bounds of basic columns tightened
  (bounded_resolve_ref.perturb "bound"), re-solved by bounded_resolve_ref.resolve; kept when the bounded dual simplex
  ends INFEASIBLE with consistent bounds.
"""
import numpy as np

from tests import bounded_ref as B
from tests import bounded_resolve_ref as BR

NONE, FARKAS, RAY = 0, 1, 2
OPTIMAL, UNBOUNDED, INFEASIBLE = 0, 1, 4

SHAPES = [(4, 12), (6, 16), (12, 32), (32, 96)]
SEEDS = range(40)


def _case(A, b, c, lo, hi, maximize, r):
    return dict(A=A, b=b, c=c, lo=lo, hi=hi, maximize=bool(maximize), basis=r["basis"], at_upper=r["at_upper"],
                run=int(r["status"]))


def cold(seed, m, n, kind, solve=B.bounded, maximize=None):
    A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n, maximize, kind=kind)
    return _case(A, b, c, lo, hi, mx, solve(A, b, c, lo, hi, mx))


def rich_unbounded_lp(seed, m, n, maximize=None):
    """(A, b, c, lo, hi, maximize): see the module docstring."""
    A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n, maximize, kind="mixed")
    no = n - m
    j = int(np.random.default_rng(31_000 + seed).integers(0, no))
    A = A.copy()
    A[:, j] = -A[:, j]
    lo[j], hi[j] = 0.0, np.inf
    hi[no:] = np.inf
    c[no:] = 0.0
    c[j] = 1.0 if mx else -1.0
    return A, b, c, lo, hi, mx


def rich_unbounded(seed, m, n, solve=B.bounded, maximize=None):
    A, b, c, lo, hi, mx = rich_unbounded_lp(seed, m, n, maximize)
    return _case(A, b, c, lo, hi, mx, solve(A, b, c, lo, hi, mx))


def dual_infeasible_lp(seed, m, n, maximize=None):
    """(A, b, c, lo2, hi2, maximize, basis, at_upper) of the perturbed re-solve, or None when the cold solve is not
    optimal."""
    A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n, maximize, kind="mixed")
    r = B.bounded(A, b, c, lo, hi, mx)
    if r["status"] != OPTIMAL:
        return None
    _, _, lo2, hi2 = BR.perturb(seed, "bound", b, c, lo, hi, r["basis"], r["x"])
    return A, b, c, lo2, hi2, mx, r["basis"], r["at_upper"]


def dual_infeasible(seed, m, n, resolve=BR.resolve, maximize=None):
    """The case, or None when the re-solve does not end INFEASIBLE with consistent bounds."""
    p = dual_infeasible_lp(seed, m, n, maximize)
    if p is None:
        return None
    A, b, c, lo2, hi2, mx, basis, up = p
    if np.any(hi2 < lo2):
        return None
    g = resolve(A, b, c, lo2, hi2, basis, up, mx)
    return _case(A, b, c, lo2, hi2, mx, g) if g["status"] == INFEASIBLE else None


def stack(cases):
    """The cases (one shape) as batch arrays: dict(A, b, c, lo, hi, basis, at_upper, run)."""
    return {k: np.stack([np.asarray(cs[k]) for cs in cases])
            for k in ("A", "b", "c", "lo", "hi", "basis", "at_upper", "run")}


def check_farkas(A, b, lo, hi, f, value):
    """f.b lies below the minimum of f^T A x over the box by about |value|."""
    assert np.all(np.isfinite(f))
    g = A.T @ f
    inf = np.isinf(hi)
    assert (g[inf] >= -1e-7).all()
    S = float(np.sum(g[inf] * lo[inf]) + np.sum(np.minimum(g[~inf] * lo[~inf], g[~inf] * hi[~inf])))
    assert f @ b < S - 1e-7, (f @ b, S)
    assert S - f @ b >= abs(value) * (1.0 - 1e-6) - 1e-7, (S - f @ b, value)


def check_ray(A, c, hi, r, value, maximize):
    """A r = 0, r >= 0, r = 0 under a finite upper bound, and c.r = value of the improving sign."""
    assert np.all(np.isfinite(r))
    assert np.abs(A @ r).max() < 1e-8
    assert (r >= -1e-8).all()
    assert (r[np.isfinite(hi)] <= 1e-8).all()
    assert (c @ r > 0) if maximize else (c @ r < 0)
    assert abs(c @ r - value) <= 1e-8


def check(cs, cert):
    """The certificate's own properties and the NaN layout of its kind."""
    if cert["kind"] == FARKAS:
        check_farkas(cs["A"], cs["b"], cs["lo"], cs["hi"], cert["farkas"], cert["value"])
        assert np.isnan(cert["ray"]).all()
        assert cert["value"] < 0
    elif cert["kind"] == RAY:
        check_ray(cs["A"], cs["c"], cs["hi"], cert["ray"], cert["value"], cs["maximize"])
        assert np.isnan(cert["farkas"]).all()
        assert cert["ray"][cert["index"]] == 1.0
    else:
        assert cert["kind"] == NONE
        assert np.isnan(cert["farkas"]).all() and np.isnan(cert["ray"]).all() and np.isnan(cert["value"])
        assert cert["index"] == -1
