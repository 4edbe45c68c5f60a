"""ctypes bindings of tests/ref/bounded_rules_ref.c and tests/ref/bounded_resolve_rules_ref.c (the bounded-variable
simplex and its re-solve under Dantzig's, Bland's or the Devex rule) and the cycling LPs the rule tests and
scripts/time_bounded_rules.py share.  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build
from tests import bland_ref

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None
_rlib = None

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
DANTZIG, BLAND, DEVEX = range(3)
RULES = (DANTZIG, BLAND, DEVEX)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_bounded_rules_ref())
        L.ref_bounded_rule.restype = C.c_int
        L.ref_bounded_rule.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double,
                                       C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int]
        _lib = L
    return _lib


def rlib():
    global _rlib
    if _rlib is None:
        L = C.CDLL(build.build_bounded_resolve_rules_ref())
        L.ref_bounded_resolve_rule.restype = C.c_int
        L.ref_bounded_resolve_rule.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int,
                                               C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int]
        _rlib = L
    return _rlib


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def bounded(A, b, c, lo, hi, maximize=False, n_orig=None, eps=1e-9, max_iter=10000, rule=DANTZIG):
    """dict(status, x (n_orig, NaN unless optimal), basis, at_upper, obj (NaN unless optimal), iters (4))."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    n_orig = n if n_orig is None else int(n_orig)
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    x = np.full(n_orig, np.nan)
    basis = np.full(m, -1, dtype=np.int32)
    up = np.zeros(n, dtype=np.int32)
    obj = C.c_double(float("nan"))
    it = np.zeros(4, dtype=np.int32)
    st = lib().ref_bounded_rule(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), int(maximize), n_orig, eps, max_iter,
                                _d(x), _i(basis), _i(up), C.byref(obj), _i(it), int(rule))
    return dict(status=st, x=x, basis=basis, at_upper=up, obj=obj.value, iters=it.tolist())


def resolve(A, b, c, lo, hi, basis, at_upper, maximize=False, n_orig=None, eps=1e-9, max_iter=10000, rule=DANTZIG):
    """dict(status, x, basis, at_upper, obj, iters (dual pivots, primal pivots, bound flips))."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    n_orig = n if n_orig is None else int(n_orig)
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    at_upper = np.ascontiguousarray(at_upper, dtype=np.int32)
    assert basis.shape == (m,) and at_upper.shape == (n,)
    x = np.full(n_orig, np.nan)
    bo = np.full(m, -1, dtype=np.int32)
    up = np.zeros(n, dtype=np.int32)
    obj = C.c_double(float("nan"))
    it = np.zeros(3, dtype=np.int32)
    st = rlib().ref_bounded_resolve_rule(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper),
                                         int(maximize), n_orig, eps, max_iter, _d(x), _i(bo), _i(up), C.byref(obj),
                                         _i(it), int(rule))
    return dict(status=st, x=x, basis=bo, at_upper=up, obj=obj.value, iters=it.tolist())


def beale_boxed(hi=100.0):
    """Beale's cycling LP (bland_ref.beale) with every column boxed to [0, hi]: (A, b, c, lo, hi, maximize)."""
    A, b, c = bland_ref.beale()[:3]
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[1]
    return A, np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64), np.zeros(n), np.full(n, float(hi))


def slack_start(A):
    """The slack basis (the last m columns) and no flag: the start of the re-solve from the slack basis."""
    m, n = A.shape
    return np.arange(n - m, n, dtype=np.int32), np.zeros(n, dtype=np.int32)


def cycling_boxed(seed=7, m=64, n=128, hi=1e3):
    """bland_ref.cycling_lp(seed, m, n) (Beale blocks beside a random block, maximise) with every column boxed to
    [0, hi]: (A, b, c, lo, hi)."""
    A, b, c = bland_ref.cycling_lp(seed, m, n)[:3]
    A = np.asarray(A, dtype=np.float64)
    return A, np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64), np.zeros(n), np.full(n, float(hi))


KINDS = ("mixed", "box", "infeasible", "unbounded", "crossed")


def seeded_lps(count=200):
    """`count` small boxed LPs of every kind of bounded_ref.boxed_lp, m = 3 .. 16: yields (A, b, c, lo, hi, maximize)."""
    from tests import bounded_ref
    for k in range(count):
        m = 3 + k % 14
        n = 2 * m + 2 + (k // 14) % 5
        yield bounded_ref.boxed_lp(k, m, n, kind=KINDS[k % 5])
