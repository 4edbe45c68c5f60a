"""ctypes binding of tests/ref/parametric_ref.c (the parametric right-hand-side path z*(t) of an LP, b + t d, from an
optimal basis) and the cases the CPU and GPU tests share.  Test infrastructure only."""
import ctypes as C

import numpy as np

from oracle import pyoracle as o
from simplexmethod_amd import build, capi
from tests import lpcases

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None

OPTIMAL, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = 0, 2, 3, 4, 5
KEYS = ("t", "obj", "slope")   # float outputs (enter, leave, basis, nseg, status: integers)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_parametric_ref())
        L.ref_parametric.restype = C.c_int
        L.ref_parametric.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, _dp, C.c_double, C.c_double,
                                     C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip]
        _lib = L
    return _lib


def parametric(A, b, c, basis, d, t_max=np.inf, maximize=True, eps=1e-9, max_breaks=64):
    """dict(status, nseg, t, obj (max_breaks+2), slope, enter, leave (max_breaks+1), basis (m)), padded with NaN / -1
    past the path (the layout of the batched C calls)."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c, d = (np.ascontiguousarray(v, dtype=np.float64) for v in (b, c, d))
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    nb = max(int(max_breaks), 0)
    t, obj, slope = np.zeros(nb + 2), np.zeros(nb + 2), np.zeros(nb + 1)
    enter, leave = np.zeros(nb + 1, np.int32), np.zeros(nb + 1, np.int32)
    bo, nseg = np.zeros(m, np.int32), C.c_int(-7)
    st = lib().ref_parametric(Af.ctypes.data_as(_dp), m, n, b.ctypes.data_as(_dp), c.ctypes.data_as(_dp),
                              basis.ctypes.data_as(_ip), int(maximize), d.ctypes.data_as(_dp), float(t_max),
                              float(eps), int(max_breaks), C.byref(nseg), t.ctypes.data_as(_dp),
                              obj.ctypes.data_as(_dp), slope.ctypes.data_as(_dp), enter.ctypes.data_as(_ip),
                              leave.ctypes.data_as(_ip), bo.ctypes.data_as(_ip))
    return dict(status=st, nseg=nseg.value, t=t, obj=obj, slope=slope, enter=enter, leave=leave, basis=bo)


def parametric_batched(A, b, c, basis, d, t_max=np.inf, maximize=True, eps=1e-9, max_breaks=64, run_status=None):
    """The reference per LP with the batched calls' padded layout; LPs whose run_status is not OPTIMAL keep it, get
    nseg 0, NaN / -1 and their basis back (lp_batched_parametric)."""
    batch, m, _ = np.shape(A)
    nb = int(max_breaks)
    out = dict(status=np.zeros(batch, np.int32), nseg=np.zeros(batch, np.int32), t=np.full((batch, nb + 2), np.nan),
               obj=np.full((batch, nb + 2), np.nan), slope=np.full((batch, nb + 1), np.nan),
               enter=np.full((batch, nb + 1), -1, np.int32), leave=np.full((batch, nb + 1), -1, np.int32),
               basis=np.array(basis, dtype=np.int32).reshape(batch, m))
    for k in range(batch):
        if run_status is not None and run_status[k] != OPTIMAL:
            out["status"][k] = run_status[k]
            continue
        r = parametric(A[k], b[k], c[k], basis[k], d[k], t_max, maximize, eps, max_breaks)
        for key in out:
            out[key][k] = r[key]
    return out


def trim(r):
    """The single-LP dict of capi.Context.basis_parametric: arrays cut to the path."""
    ns = r["nseg"]
    return dict(status=r["status"], t=r["t"][:ns + 1] if ns else r["t"][:0], obj=r["obj"][:ns + 1] if ns else r["obj"][:0],
                slope=r["slope"][:ns], enter=r["enter"][:ns], leave=r["leave"][:ns], basis=r["basis"])


# ---- cases ---------------------------------------------------------------------------------------------------------

def direction(seed, b, scale=1.0):
    """Seeded direction with mixed signs, scaled by |b|."""
    rng = np.random.default_rng(7919 + seed)
    return rng.uniform(-1.0, 1.0, size=len(b)) * np.abs(b) * scale


def max_case(seed, m, n):
    """capi.gen_lp (max) at the oracle's optimal basis with a seeded direction: (A, b, c, basis, d, maximize)."""
    A, b, c, basis = capi.gen_lp(seed, m, n)
    r = o.simplex_tableau(A, b, c, basis, True, n)
    assert r["status"] == OPTIMAL
    return A, b, c, np.asarray(r["basis"], np.int32), direction(seed, b), True


def min_case(seed, m, k):
    """lpcases.min_lp (min) at the oracle's two-phase optimal basis with a seeded direction."""
    A, b, c, _ = lpcases.min_lp(seed, m, k)
    r = o.two_phase(A, b, c, False, A.shape[1])
    assert r["status"] == OPTIMAL
    return A, b, c, np.asarray(r["basis"], np.int32), direction(seed, b), False


def zero_length_case():
    """max 2 x1 + 2 x2 - 4 y with x1 - y <= 1, x2 - y/2 <= 1, y <= 5 at its optimum {x1, x2, s2} (y = 0), moved
    along d = (-1, -1, 0): x1 and x2 reach 0 together at t = 1, y enters on x1's row and x2 blocks again at the same
    t, so the path holds a segment of length 0."""
    A = np.array([[1.0, 0.0, -1.0, 1.0, 0.0, 0.0],
                  [0.0, 1.0, -0.5, 0.0, 1.0, 0.0],
                  [0.0, 0.0, 1.0, 0.0, 0.0, 1.0]])
    b = np.array([1.0, 1.0, 5.0])
    c = np.array([2.0, 2.0, -4.0, 0.0, 0.0, 0.0])
    basis = np.array([0, 1, 5], np.int32)
    d = np.array([-1.0, -1.0, 0.0])
    return A, b, c, basis, d, True


def infeasible_case():
    """capi.gen_lp 12 x 30 at its optimum, b shrunk towards 0 and past it: infeasible for every t > 1."""
    A, b, c, basis, _, mx = max_case(3, 12, 30)
    return A, b, c, basis, -b.copy(), mx


def unbounded_t_case():
    """capi.gen_lp 10 x 24 at its optimum, b grown: feasible for every t >= 0, the path ends at +inf."""
    A, b, c, basis, _, mx = max_case(4, 10, 24)
    return A, b, c, basis, np.abs(direction(4, b)) + 0.25 * b, mx


def named_cases():
    """name -> (A, b, c, basis, d, maximize)."""
    return {
        "max_8x20": max_case(11, 8, 20),
        "max_16x40": max_case(12, 16, 40),
        "max_24x48": max_case(13, 24, 48),
        "min_6x16": min_case(14, 6, 10),
        "min_12x32": min_case(15, 12, 20),
        "zero_length": zero_length_case(),
        "infeasible_end": infeasible_case(),
        "unbounded_t": unbounded_t_case(),
    }
