"""ctypes binding of tests/ref/resolve_ref.c (the re-solve of an LP from a given basis: the oracle's
primal loop when the basis is primal feasible, the dual simplex when it is only dual feasible) and the
perturbed LPs the re-solve tests and scripts/time_resolve.py share.  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build, capi

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_resolve_ref())
        L.ref_resolve.restype = C.c_int
        L.ref_resolve.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int, C.c_double, C.c_int,
                                  _dp, _ip, _dp, _ip, _ip, _ip, C.c_int, _dp]
        _lib = L
    return _lib


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def resolve(A, b, c, basis, maximize=True, n_orig=None, eps=1e-9, max_iter=10000, trace_cap=0,
            want_tableau=False):
    """dict(status, x, basis, obj, iters=(dual, primal), trace=[(enter, leave)...], tableau)."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    n_orig = n if n_orig is None else n_orig
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    x = np.zeros(max(n_orig, 1))
    bo = np.zeros(m, dtype=np.int32)
    obj = C.c_double(float("nan"))
    it = np.zeros(2, dtype=np.int32)
    te = np.full(max(trace_cap, 1), -1, dtype=np.int32)
    tl = np.full(max(trace_cap, 1), -1, dtype=np.int32)
    tab = np.zeros((m + 1, n + 1)) if want_tableau else None
    st = lib().ref_resolve(_d(Af), m, n, _d(b), _d(c), _i(basis), int(maximize), n_orig, eps, max_iter, _d(x),
                           _i(bo), C.byref(obj), _i(it), _i(te), _i(tl), trace_cap, _d(tab))
    k = min(int(it.sum()), trace_cap)
    return dict(status=st, x=x[:n_orig], basis=bo, obj=obj.value, iters=(int(it[0]), int(it[1])),
                trace=list(zip(te[:k].tolist(), tl[:k].tolist())), tableau=tab)


def scale_rows(seed, b, lo=0.3, hi=0.9):
    """b with 1-4 seeded rows scaled by a seeded factor in [lo, hi]: the old optimal basis of an LP whose
    b shrank usually has some xB < 0 (primal infeasible) and is still dual feasible."""
    rng = np.random.default_rng(seed)
    b = np.array(b, dtype=np.float64)
    k = int(rng.integers(1, 5))
    rows = rng.choice(len(b), size=min(k, len(b)), replace=False)
    b[rows] *= rng.uniform(lo, hi, size=len(rows))
    return b


def scenario(batch, m, n, seed0=0):
    """The timing scenario: `batch` LPs gen_lp(seed0 + k, m, n) and their perturbed right-hand sides.
    Returns (A (batch, m, n), b (batch, m), b' (batch, m), c (batch, n), slack bases (batch, m))."""
    A = np.empty((batch, m, n))
    b = np.empty((batch, m))
    c = np.empty((batch, n))
    basis = np.empty((batch, m), dtype=np.int32)
    for k in range(batch):
        A[k], b[k], c[k], basis[k] = capi.gen_lp(seed0 + k, m, n)
    b2 = np.stack([scale_rows(10_000 + seed0 + k, b[k]) for k in range(batch)])
    return A, b, b2, c, basis
