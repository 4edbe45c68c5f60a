"""ctypes binding of tests/ref/mip_ref.c (depth-first branch-and-bound from a given root basis) and the small
integer problems the MIP tests and scripts/time_mip.py share.  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_mip_ref())
        L.ref_mip.restype = C.c_int
        L.ref_mip.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int, _ip, C.c_double, C.c_double,
                              C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip]
        _lib = L
    return _lib


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def mip(A, b, c, basis, integer, maximize=True, n_orig=None, eps=1e-9, int_tol=1e-6, gap=1e-9, max_depth=32,
        max_nodes=100000, max_iter=10000):
    """dict(status, found, x, obj, bound, stats=(nodes, dual pivots, primal pivots, deepest level))."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    n_orig = n if n_orig is None else n_orig
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    integer = np.ascontiguousarray(integer, dtype=np.int32)
    x = np.zeros(max(n_orig, 1))
    obj, bound = C.c_double(0.0), C.c_double(0.0)
    found = C.c_int(0)
    stats = np.zeros(4, dtype=np.int32)
    st = lib().ref_mip(_d(Af), m, n, _d(b), _d(c), _i(basis), int(maximize), n_orig, _i(integer), eps, int_tol, gap,
                       max_depth, max_nodes, max_iter, _d(x), C.byref(obj), C.byref(bound), C.byref(found),
                       _i(stats))
    return dict(status=st, found=found.value, x=x[:n_orig], obj=obj.value, bound=bound.value,
                stats=tuple(int(s) for s in stats))


def knapsack(seed, m, k, box=3):
    """A pure-integer max problem [A | I] x = b with A, b, c > 0: m rows, k integer columns, each x_j <= box by
    construction of b.  Returns (A (m, k+m), b, c (zero on the slacks), slack basis, mask)."""
    rng = np.random.default_rng(seed)
    A0 = rng.uniform(1.0, 9.0, size=(m, k)).round(2)
    b = np.array([rng.uniform(0.3, 0.8) * A0[i].sum() * box / 2 for i in range(m)]).round(3)
    c0 = rng.uniform(1.0, 9.0, size=k).round(2)
    A = np.hstack([A0, np.eye(m)])
    c = np.concatenate([c0, np.zeros(m)])
    basis = np.arange(k, k + m, dtype=np.int32)
    mask = np.concatenate([np.ones(k, dtype=np.int32), np.zeros(m, dtype=np.int32)])
    return A, b, c, basis, mask


def brute_force(A0, b, c0):
    """max c0.x over integer x >= 0 with A0 x <= b, by enumeration (A0, b, c0 > 0).  (obj or None, x or None)."""
    k = A0.shape[1]
    ub = [int(np.floor(min(b[i] / A0[i, j] for i in range(A0.shape[0])))) for j in range(k)]
    best, bx = None, None
    grids = np.meshgrid(*[np.arange(u + 1) for u in ub], indexing="ij")
    X = np.stack([g.reshape(-1) for g in grids], axis=1).astype(np.float64)
    ok = np.all(X @ A0.T <= b + 1e-9, axis=1)
    if ok.any():
        vals = X[ok] @ c0
        i = int(np.argmax(vals))
        best, bx = float(vals[i]), X[ok][i]
    return best, bx
