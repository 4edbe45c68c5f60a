"""ctypes binding of tests/ref/mip_bounded_ref.c (depth-first branch-and-bound over variable bounds from a given basis
and given complement flags) and the boxed integer problems the bounded-MIP tests and scripts/time_mip_bounded.py
share.  Test infrastructure only."""
import ctypes as C
import itertools

import numpy as np

from simplexmethod_amd import build
from tests import bounded_ref as B
from tests import mip_ref as M

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_mip_bounded_ref())
        L.ref_mip_bounded.restype = C.c_int
        L.ref_mip_bounded.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int, _ip,
                                      C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp,
                                      _ip, _ip]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def mip(A, b, c, lo, hi, basis, at_upper, integer, maximize=True, n_orig=None, eps=1e-9, int_tol=1e-6, gap=1e-9,
        max_depth=64, max_nodes=100000, max_iter=10000):
    """dict(status, found, x (n_orig, NaN without an incumbent), obj, bound, stats=(nodes, dual pivots, primal pivots,
    bound flips, deepest level))."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    n_orig = n if n_orig is None else int(n_orig)
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    at_upper = np.ascontiguousarray(at_upper, dtype=np.int32)
    integer = np.ascontiguousarray(integer, dtype=np.int32)
    assert basis.shape == (m,) and at_upper.shape == (n,) and integer.shape == (n,)
    x = np.zeros(max(n_orig, 1))
    obj, bound = C.c_double(0.0), C.c_double(0.0)
    found = C.c_int(0)
    stats = np.zeros(5, dtype=np.int32)
    st = lib().ref_mip_bounded(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize),
                               n_orig, _i(integer), eps, int_tol, gap, max_depth, max_nodes, max_iter, _d(x),
                               C.byref(obj), C.byref(bound), C.byref(found), _i(stats))
    return dict(status=st, found=found.value, x=x[:n_orig], obj=obj.value, bound=bound.value,
                stats=tuple(int(s) for s in stats))


def boxed_knapsack(seed, m, k):
    """mip_ref.knapsack(seed, m, k) plus integer boxes on the k integer columns: lo_j in {0, 1} (1 for one column in
    five), hi_j in {1, 2, 3} (at most 2 when k > 7), the slacks in [0, inf).  Returns (A, b, c, lo, hi, mask, root) with
    root the cold bounded_ref.bounded result (max)."""
    A, b, c, _, mask = M.knapsack(seed, m, k)
    rng = np.random.default_rng(50000 + seed)
    n = k + m
    lo, hi = np.zeros(n), np.full(n, np.inf)
    lo[:k] = rng.random(k) < 0.2
    hi[:k] = np.maximum(lo[:k], rng.integers(1, 3 if k > 7 else 4, k))
    root = B.bounded(A, b, c, lo, hi, True)
    return A, b, c, lo, hi, mask, root


def enumerate_box(A0, b, c0, lo, hi):
    """max c0.x over integer lo <= x <= hi with A0 x <= b, by enumeration.  (obj or None, x or None)."""
    ranges = [np.arange(int(l), int(h) + 1) for l, h in zip(lo, hi)]
    X = np.array(list(itertools.product(*ranges)), dtype=np.float64)
    ok = np.all(X @ A0.T <= b + 1e-9, axis=1)
    if not ok.any():
        return None, None
    vals = X[ok] @ c0
    i = int(np.argmax(vals))
    return float(vals[i]), X[ok][i]


def milp(A, b, c, lo, hi, integer, maximize):
    """scipy.optimize.milp on the same problem with mip_rel_gap = 0: (status OPTIMAL / INFEASIBLE / UNBOUNDED, obj)."""
    from scipy.optimize import Bounds, LinearConstraint, milp as sp_milp
    sign = -1.0 if maximize else 1.0
    r = sp_milp(sign * np.asarray(c), constraints=LinearConstraint(A, b, b), integrality=np.asarray(integer),
                bounds=Bounds(lo, hi), options=dict(mip_rel_gap=0.0))
    if r.status == 0:
        return OPTIMAL, sign * r.fun
    return {2: INFEASIBLE, 3: UNBOUNDED}.get(r.status, -1), None


def boxed_mip(seed, m, n, maximize=None, kind="mixed", every=1):
    """bounded_ref.boxed_lp(seed, m, n, maximize, kind) with every `every`-th structural column integer and the marked
    columns' bounds rounded outward to integers.  Returns (A, b, c, lo, hi, mask, maximize)."""
    A, b, c, lo, hi, maximize = B.boxed_lp(seed, m, n, maximize=maximize, kind=kind)
    mask = np.zeros(n, dtype=np.int32)
    mask[0:n - m:every] = 1
    lo, hi = lo.copy(), hi.copy()
    for j in np.flatnonzero(mask):
        lo[j] = np.floor(lo[j])
        if np.isfinite(hi[j]):
            hi[j] = np.ceil(hi[j])
    return A, b, c, lo, hi, mask, maximize


def mixed_case(seed, m=5, n=14):
    """boxed_mip(seed, m, n, kind="mixed") with every other structural column integer, and its cold root by
    bounded_ref.bounded.  Returns (A, b, c, lo, hi, mask, maximize, root)."""
    A, b, c, lo, hi, mask, maximize = boxed_mip(seed, m, n, kind="mixed", every=2)
    root = B.bounded(A, b, c, lo, hi, maximize)
    return A, b, c, lo, hi, mask, maximize, root


DEEP_SEED, DEEP_K = 2, 120


def deep_case():
    """A seed-pinned binary knapsack (one row, 120 integer columns in [0, 1], costs close to the weights) whose search,
    by the reference, solves nodes above level 64, the row form's cap: about 2100 nodes, deepest level 77.  Returns
    (A, b, c, lo, hi, mask, maximize, root) with root the cold bounded_ref.bounded result."""
    rng = np.random.default_rng(DEEP_SEED)
    k, m = DEEP_K, 1
    A0 = rng.uniform(1.0, 9.0, size=(m, k)).round(2)
    b = (A0.sum(axis=1) * rng.uniform(0.3, 0.7, m)).round(3)
    c0 = (A0.mean(axis=0) + rng.uniform(-2.0, 2.0, k)).round(2)
    A = np.hstack([A0, np.eye(m)])
    c = np.concatenate([c0, np.zeros(m)])
    n = k + m
    lo, hi = np.zeros(n), np.full(n, np.inf)
    hi[:k] = 1.0
    mask = np.concatenate([np.ones(k, dtype=np.int32), np.zeros(m, dtype=np.int32)])
    root = B.bounded(A, b, c, lo, hi, True)
    return A, b, c, lo, hi, mask, True, root
