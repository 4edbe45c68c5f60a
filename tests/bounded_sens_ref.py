"""ctypes binding of tests/ref/bounded_sens_ref.c (the dual solution and RHS / cost ranging of a bounded-variable LP at
a given basis and given at-upper flags) and small helpers the bounded sensitivity tests and
scripts/time_bounded_sens.py share.  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)

DUALS_KEYS = ("x", "y", "d", "w")
RANGING_KEYS = ("b_lo", "b_hi", "b_leave", "b_side", "c_lo", "c_hi", "c_enter")


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_bounded_sens_ref())
        L.ref_bounded_duals.restype = C.c_int
        L.ref_bounded_duals.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _dp]
        L.ref_bounded_ranging.restype = C.c_int
        L.ref_bounded_ranging.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_double,
                                          _dp, _ip, _ip, _dp, _ip]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _in(A, b, c, lo, hi, basis, at_upper):
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Af = np.ascontiguousarray(A.T).reshape(-1)
    f = [np.ascontiguousarray(v, dtype=np.float64) for v in (b, c, lo, hi)]
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    at_upper = np.ascontiguousarray(at_upper, dtype=np.int32)
    assert basis.shape == (m,) and at_upper.shape == (n,)
    return m, n, Af, f[0], f[1], f[2], f[3], basis, at_upper


def split(status, rhs, rhs_var, rhs_side, cost, cost_var):
    """Interleaved pairs -> dict(status, b_lo, b_hi, b_leave (m x 2), b_side (m x 2), c_lo, c_hi, c_enter (n x 2))."""
    pair = lambda a: a.reshape(a.shape[:-1] + (-1, 2))
    return dict(status=status, b_lo=rhs[..., 0::2], b_hi=rhs[..., 1::2], b_leave=pair(rhs_var), b_side=pair(rhs_side),
                c_lo=cost[..., 0::2], c_hi=cost[..., 1::2], c_enter=pair(cost_var))


def duals(A, b, c, lo, hi, basis, at_upper):
    """dict(status, x (n), y (m), d (n), w); NaN unless status is OPTIMAL."""
    m, n, Af, b, c, lo, hi, basis, at_upper = _in(A, b, c, lo, hi, basis, at_upper)
    x, y, d = np.zeros(n), np.zeros(m), np.zeros(n)
    w = C.c_double(0.0)
    st = lib().ref_bounded_duals(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), _d(x), _d(y),
                                 _d(d), C.byref(w))
    return dict(status=st, x=x, y=y, d=d, w=w.value)


def ranging(A, b, c, lo, hi, basis, at_upper, maximize=False, eps=1e-9):
    """dict as split(); NaN and -1 unless status is OPTIMAL."""
    m, n, Af, b, c, lo, hi, basis, at_upper = _in(A, b, c, lo, hi, basis, at_upper)
    rhs, cost = np.zeros(2 * m), np.zeros(2 * n)
    rv, rs, cv = np.zeros(2 * m, np.int32), np.zeros(2 * m, np.int32), np.zeros(2 * n, np.int32)
    st = lib().ref_bounded_ranging(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize),
                                   float(eps), _d(rhs), _i(rv), _i(rs), _d(cost), _i(cv))
    return split(st, rhs, rv, rs, cost, cv)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, keys):
    """Every key of `want` equals `got` bit for bit (floats: NaN where NaN, signed zeros included)."""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if w.dtype.kind == "f":
            assert np.array_equal(bits(g), bits(w)), k
        else:
            assert np.array_equal(g, w), k


def batched(fn, A, b, c, lo, hi, basis, at_upper, *args):
    """The reference per LP, stacked along a leading batch axis."""
    rs = [fn(A[k], b[k], c[k], lo[k], hi[k], basis[k], at_upper[k], *args) for k in range(len(A))]
    return {key: np.stack([np.asarray(r[key]) for r in rs]) for key in rs[0]}
