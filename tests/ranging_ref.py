"""ctypes binding of tests/ref/ranging_ref.c (RHS and cost ranging of an LP at a given basis: the crash on
[B | I | b] for B^-1 and xB, the reduced costs of duals_ref.c, the alpha = B^-1 A_N chains and the ratio
reductions).  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_ranging_ref())
        L.ref_ranging.restype = C.c_int
        L.ref_ranging.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_double, _dp, _ip, _dp, _ip]
        L.ref_ranging_crash.restype = C.c_int
        L.ref_ranging_crash.argtypes = [_dp, C.c_int, C.c_int, _dp, _ip, C.c_int, _dp, _dp]
        _lib = L
    return _lib


def _in(A, b, c, basis):
    A = np.asarray(A, dtype=np.float64)
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    return A.shape, Af, b, c, np.ascontiguousarray(basis, dtype=np.int32)


def split(status, rhs, rhs_var, cost, cost_var):
    """Interleaved pairs -> dict(status, b_lo, b_hi, b_leave (m x 2), c_lo, c_hi, c_enter (n x 2))."""
    return dict(status=status, b_lo=rhs[..., 0::2], b_hi=rhs[..., 1::2],
                b_leave=rhs_var.reshape(rhs_var.shape[:-1] + (-1, 2)),
                c_lo=cost[..., 0::2], c_hi=cost[..., 1::2], c_enter=cost_var.reshape(cost_var.shape[:-1] + (-1, 2)))


def ranging(A, b, c, basis, maximize=True, eps=1e-9):
    """dict as capi.Context.basis_ranging; NaN and -1 unless status is OPTIMAL (0)."""
    (m, n), Af, b, c, basis = _in(A, b, c, basis)
    rhs, cost = np.zeros(2 * m), np.zeros(2 * n)
    rv, cv = np.zeros(2 * m, np.int32), np.zeros(2 * n, np.int32)
    st = lib().ref_ranging(Af.ctypes.data_as(_dp), m, n, b.ctypes.data_as(_dp), c.ctypes.data_as(_dp),
                           basis.ctypes.data_as(_ip), int(maximize), float(eps), rhs.ctypes.data_as(_dp),
                           rv.ctypes.data_as(_ip), cost.ctypes.data_as(_dp), cv.ctypes.data_as(_ip))
    return split(st, rhs, rv, cost, cv)


def crash(A, b, basis, inplace):
    """(status, Binv (m x m, rows by basis position), xB) of step 1, explicit or in-place form."""
    A = np.asarray(A, dtype=np.float64)
    (m, n), Af, b, _, basis = _in(A, b, np.zeros(A.shape[1]), basis)
    binv, xb = np.full((m, m), np.nan), np.full(m, np.nan)
    st = lib().ref_ranging_crash(Af.ctypes.data_as(_dp), m, n, b.ctypes.data_as(_dp), basis.ctypes.data_as(_ip),
                                 int(inplace), binv.ctypes.data_as(_dp), xb.ctypes.data_as(_dp))
    return st, binv, xb


def ranging_batched(A, b, c, basis, maximize=True, eps=1e-9, run_status=None):
    """The reference per LP; LPs whose run_status is not OPTIMAL keep it and get NaN (lp_batched_ranging)."""
    batch, m, n = np.shape(A)
    out = dict(status=np.zeros(batch, np.int32), b_lo=np.full((batch, m), np.nan), b_hi=np.full((batch, m), np.nan),
               b_leave=np.full((batch, m, 2), -1, np.int32), c_lo=np.full((batch, n), np.nan),
               c_hi=np.full((batch, n), np.nan), c_enter=np.full((batch, n, 2), -1, np.int32))
    for k in range(batch):
        if run_status is not None and run_status[k] != 0:
            out["status"][k] = run_status[k]
            continue
        r = ranging(A[k], b[k], c[k], basis[k], maximize, eps)
        for key in out:
            out[key][k] = r[key]
    return out
