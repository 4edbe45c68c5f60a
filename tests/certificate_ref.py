"""ctypes binding of tests/ref/certificate_ref.c (Farkas and unbounded-ray certificates of an LP at a given basis:
the ranging crash on [B | I | b] with artificial columns, then the phase-I, dual-simplex or ray case).  Test
infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_certificate_ref())
        L.ref_certificate.restype = C.c_int
        L.ref_certificate.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_double, _ip, _dp, _dp, _dp,
                                      _ip]
        L.ref_certificate_crash.restype = C.c_int
        L.ref_certificate_crash.argtypes = [_dp, C.c_int, C.c_int, _dp, _ip, C.c_double, _dp, _dp]
        _lib = L
    return _lib


def _in(A, b, c, basis):
    A = np.asarray(A, dtype=np.float64)
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    return A.shape, Af, b, c, np.ascontiguousarray(basis, dtype=np.int32)


def certificate(A, b, c, basis, maximize=True, eps=1e-9):
    """dict as capi.Context.basis_certificate (status instead of an exception for BAD_ARG)."""
    (m, n), Af, b, c, basis = _in(A, b, c, basis)
    kind, index = np.zeros(1, np.int32), np.zeros(1, np.int32)
    farkas, ray, value = np.zeros(m), np.zeros(n), np.zeros(1)
    st = lib().ref_certificate(Af.ctypes.data_as(_dp), m, n, b.ctypes.data_as(_dp), c.ctypes.data_as(_dp),
                               basis.ctypes.data_as(_ip), int(maximize), float(eps), kind.ctypes.data_as(_ip),
                               farkas.ctypes.data_as(_dp), ray.ctypes.data_as(_dp), value.ctypes.data_as(_dp),
                               index.ctypes.data_as(_ip))
    return dict(status=st, kind=int(kind[0]), farkas=farkas, ray=ray, value=float(value[0]), index=int(index[0]))


def crash(A, b, basis, eps=1e-9):
    """(status, Binv (m x m, rows by basis position), xB) of step 1."""
    A = np.asarray(A, dtype=np.float64)
    (m, n), Af, b, _, basis = _in(A, b, np.zeros(A.shape[1]), basis)
    binv, xb = np.full((m, m), np.nan), np.full(m, np.nan)
    st = lib().ref_certificate_crash(Af.ctypes.data_as(_dp), m, n, b.ctypes.data_as(_dp), basis.ctypes.data_as(_ip),
                                     float(eps), binv.ctypes.data_as(_dp), xb.ctypes.data_as(_dp))
    return st, binv, xb


def certificate_batched(A, b, c, basis, maximize=True, eps=1e-9, run_status=None):
    """The reference per LP.  With run_status (lp_batched_certificates): only LPs whose entry is INFEASIBLE (4) or
    UNBOUNDED (1) get a certificate and keep that entry as their status unless the certificate's own status is not
    OPTIMAL; the others keep their entry and get NONE."""
    batch, m, n = np.shape(A)
    out = dict(status=np.zeros(batch, np.int32), kind=np.zeros(batch, np.int32), farkas=np.full((batch, m), np.nan),
               ray=np.full((batch, n), np.nan), value=np.full(batch, np.nan), index=np.full(batch, -1, np.int32))
    for k in range(batch):
        if run_status is not None and run_status[k] not in (1, 4):
            out["status"][k] = run_status[k]
            continue
        r = certificate(A[k], b[k], c[k], basis[k], maximize, eps)
        for key in out:
            out[key][k] = r[key]
        if run_status is not None and r["status"] == 0:
            out["status"][k] = run_status[k]
    return out
