"""ctypes binding of tests/ref/bounded_resolve_long_step_ref.c: the bounded re-solve under a pivot rule (its primal
branch), a dual pricing rule (the leaving choice of its dual branch) and a dual ratio test (the entering step of that
branch: textbook, or bound-flipping).  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
DANTZIG, BLAND, DEVEX = range(3)
RULES = (DANTZIG, BLAND, DEVEX)
DUAL_DANTZIG, DUAL_DEVEX = range(2)
DUAL_RULES = (DUAL_DANTZIG, DUAL_DEVEX)
TEXTBOOK, LONG_STEP = range(2)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_bounded_resolve_long_step_ref())
        L.ref_bounded_resolve_long_step.restype = C.c_int
        L.ref_bounded_resolve_long_step.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                    C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int,
                                                    C.c_int, C.c_int]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def resolve(A, b, c, lo, hi, basis, at_upper, maximize=False, n_orig=None, eps=1e-9, max_iter=10000, rule=DANTZIG,
            dual_rule=DUAL_DANTZIG, dual_ratio=LONG_STEP):
    """dict(status, x, basis, at_upper, obj, iters (dual pivots, primal pivots, bound flips of either loop)).  The
    outputs start as x NaN, basis -1, at_upper 0, obj NaN, iters 0: what a refusal that writes nothing leaves."""
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
    st = lib().ref_bounded_resolve_long_step(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper),
                                             int(maximize), n_orig, eps, max_iter, _d(x), _i(bo), _i(up),
                                             C.byref(obj), _i(it), int(rule), int(dual_rule), int(dual_ratio))
    return dict(status=st, x=x, basis=bo, at_upper=up, obj=obj.value, iters=it.tolist())
