"""ctypes binding of tests/ref/mip_bounded_long_step_ref.c: the search of mip_bounded_snapshots_ref.c with a choice of
the ratio test of its dual loops, the definition of the lp_mip_bounded_solve_ratio_ex family.  Test infrastructure
only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build

TEXTBOOK, LONG_STEP = 0, 1
DIAG = ("restored_infeasible", "flips_root", "flips_first", "flips_rebuilt", "flips_restored", "infeasible_after_flip",
        "dual_iter_limit", "dual_loops")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_mip_bounded_long_step_ref())
        L.ref_mip_bounded_long_step.restype = C.c_int
        L.ref_mip_bounded_long_step.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int,
                                                _ip, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                                _dp, _dp, _dp, _ip, _ip, C.c_int, _ip, C.c_int]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def mip(A, b, c, lo, hi, basis, at_upper, integer, maximize=True, n_orig=None, eps=1e-9, int_tol=1e-6, gap=1e-9,
        max_depth=64, max_nodes=100000, max_iter=10000, snapshots=0, dual_ratio=LONG_STEP):
    """dict(status, found, x (n_orig, NaN without an incumbent), obj, bound, stats=(nodes, dual pivots, primal pivots,
    bound flips, deepest level, second children restored, second children rebuilt), diag=dict over DIAG)."""
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
    stats = np.zeros(7, dtype=np.int32)
    diag = np.zeros(8, dtype=np.int32)
    st = lib().ref_mip_bounded_long_step(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper),
                                         int(maximize), n_orig, _i(integer), eps, int_tol, gap, max_depth, max_nodes,
                                         max_iter, _d(x), C.byref(obj), C.byref(bound), C.byref(found), _i(stats),
                                         int(snapshots), _i(diag), int(dual_ratio))
    return dict(status=st, found=found.value, x=x[:n_orig], obj=obj.value, bound=bound.value,
                stats=tuple(int(s) for s in stats), diag=dict(zip(DIAG, (int(v) for v in diag))))
