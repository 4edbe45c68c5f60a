"""ctypes binding of tests/ref/devex_ref.c (the tableau simplex and the two-phase flow of the oracle
restated with a pivot-rule argument: 0 = Dantzig, 2 = Devex) and the badly scaled LP family the Devex
tests share.  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build, capi
from tests import lpcases

DANTZIG, DEVEX = 0, 2

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_test_devex_ref())
        L.ref_simplex_tableau.restype = C.c_int
        L.ref_simplex_tableau.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int, C.c_double,
                                          C.c_int, C.c_int, _dp, _ip, _dp, _ip, _ip, _ip, C.c_int, _dp, _dp]
        L.ref_two_phase.restype = C.c_int
        L.ref_two_phase.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_int,
                                    C.c_int, _dp, _ip, _dp, _ip]
        _lib = L
    return _lib


def _colmajor(A):
    return np.ascontiguousarray(np.asarray(A, dtype=np.float64).T).reshape(-1)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def simplex_tableau(A, b, c, basis, maximize=True, n_orig=None, rule=DEVEX, eps=1e-9, max_iter=10000,
                    trace_cap=0, want_tableau=False):
    """Same dict as oracle.pyoracle.simplex_tableau, plus `weights`: the n Devex weights when the loop
    ended (all 1.0 under Dantzig's rule)."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    n_orig = n if n_orig is None else n_orig
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    x = np.zeros(max(n_orig, 1))
    bo = np.zeros(m, dtype=np.int32)
    obj = C.c_double(float("nan"))
    it = C.c_int(0)
    te = np.full(max(trace_cap, 1), -1, dtype=np.int32)
    tl = np.full(max(trace_cap, 1), -1, dtype=np.int32)
    tab = np.zeros((m + 1, n + 1)) if want_tableau else None
    w = np.full(n, np.nan)
    st = lib().ref_simplex_tableau(_d(_colmajor(A)), m, n, _d(b), _d(c), _i(basis), int(maximize), n_orig, eps,
                                   max_iter, int(rule), _d(x), _i(bo), C.byref(obj), C.byref(it), _i(te), _i(tl),
                                   trace_cap, _d(tab), _d(w))
    k = min(it.value, trace_cap)
    return dict(status=st, x=x[:n_orig], basis=bo, obj=obj.value, iters=it.value,
                trace=list(zip(te[:k].tolist(), tl[:k].tolist())), tableau=tab, weights=w)


def two_phase(A, b, c, maximize=False, n_orig=None, rule=DEVEX, eps=1e-9, max_iter=10000):
    """Same dict as oracle.pyoracle.two_phase."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    n_orig = n if n_orig is None else n_orig
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    x = np.zeros(n_orig)
    bo = np.full(m, -1, dtype=np.int32)
    obj = C.c_double(float("nan"))
    it = np.zeros(3, dtype=np.int32)
    st = lib().ref_two_phase(_d(_colmajor(A)), m, n, _d(b), _d(c), int(maximize), n_orig, eps, max_iter, int(rule),
                             _d(x), _i(bo), C.byref(obj), _i(it))
    return dict(status=st, x=x, basis=bo, obj=obj.value, iters=it.tolist())


def scaled_lp(seed, m, n):
    """capi.gen_lp(seed, m, n) with each original column j of A and c_j multiplied by 10**U(-2, 2): the
    vertices' geometry is unchanged (x_j is measured in another unit), the reduced costs Dantzig's rule
    compares are not.  Returns (A, b, c, basis)."""
    A, b, c, basis = capi.gen_lp(seed, m, n)
    rng = np.random.default_rng(seed)
    s = 10.0 ** rng.uniform(-2.0, 2.0, size=n - m)
    A = A.copy()
    c = c.copy()
    A[:, :n - m] *= s
    c[:n - m] *= s
    return A, b, c, basis


def scaled_min_lp(seed, m, k, **kw):
    """tests/lpcases.min_lp with each original column j of A and c_j multiplied by 10**U(-2, 2)."""
    A, b, c, no = lpcases.min_lp(seed, m, k, **kw)
    rng = np.random.default_rng(seed)
    s = 10.0 ** rng.uniform(-2.0, 2.0, size=k)
    A = A.copy()
    c = c.copy()
    A[:, :k] *= s
    c[:k] *= s
    return A, b, c, no
