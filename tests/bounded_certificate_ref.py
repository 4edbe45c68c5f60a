"""ctypes binding of tests/ref/bounded_certificate_ref.c (Farkas and unbounded-ray certificates of a bounded-variable LP
at a given basis and given at-upper flags).  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
NONE, FARKAS, RAY = 0, 1, 2
KEYS = ("status", "kind", "farkas", "ray", "value", "index")


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_bounded_certificate_ref())
        L.ref_bounded_certificate.restype = C.c_int
        L.ref_bounded_certificate.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_double,
                                              _ip, _dp, _dp, _dp, _ip]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def certificate(A, b, c, lo, hi, basis, at_upper, maximize=False, eps=1e-9):
    """dict as capi.Context.basis_bounded_certificate (status instead of an exception for BAD_ARG)."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c, lo, hi = (np.ascontiguousarray(v, dtype=np.float64) for v in (b, c, lo, hi))
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    at_upper = np.ascontiguousarray(at_upper, dtype=np.int32)
    assert basis.shape == (m,) and at_upper.shape == (n,)
    kind, index = np.zeros(1, np.int32), np.zeros(1, np.int32)
    farkas, ray, value = np.zeros(m), np.zeros(n), np.zeros(1)
    st = lib().ref_bounded_certificate(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper),
                                       int(maximize), float(eps), _i(kind), _d(farkas), _d(ray), _d(value), _i(index))
    return dict(status=st, kind=int(kind[0]), farkas=farkas, ray=ray, value=float(value[0]), index=int(index[0]))


def certificate_batched(A, b, c, lo, hi, basis, at_upper, maximize=False, eps=1e-9, run_status=None):
    """The reference per LP.  With run_status (lp_basis_bounded_certificate_batched): only LPs whose entry is
    INFEASIBLE (4) or UNBOUNDED (1) get a certificate and keep that entry as their status unless the certificate's own
    status is not OPTIMAL; the others keep their entry and get NONE."""
    batch, m, n = np.shape(A)
    out = dict(status=np.zeros(batch, np.int32), kind=np.zeros(batch, np.int32), farkas=np.full((batch, m), np.nan),
               ray=np.full((batch, n), np.nan), value=np.full(batch, np.nan), index=np.full(batch, -1, np.int32))
    for k in range(batch):
        if run_status is not None and run_status[k] not in (UNBOUNDED, INFEASIBLE):
            out["status"][k] = run_status[k]
            continue
        r = certificate(A[k], b[k], c[k], lo[k], hi[k], basis[k], at_upper[k], maximize, eps)
        for key in out:
            out[key][k] = r[key]
        if run_status is not None and r["status"] == OPTIMAL:
            out["status"][k] = run_status[k]
    return out


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, keys=KEYS):
    """Every key of `want` equals `got` bit for bit (floats: NaN where NaN, signed zeros included)."""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if w.dtype.kind == "f":
            assert np.array_equal(bits(g), bits(w)), k
        else:
            assert np.array_equal(g, w), k
