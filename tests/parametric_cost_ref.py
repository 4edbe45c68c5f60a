"""ctypes binding of tests/ref/parametric_cost_ref.c (the parametric cost path z*(t) of an LP, c + t g, from an optimal
basis) and the cases the CPU and GPU tests share.  Test infrastructure only."""
import ctypes as C

import numpy as np

from oracle import pyoracle as o
from simplexmethod_amd import build, capi
from tests import lpcases

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, BAD_ARG = 0, 1, 2, 3, 5
KEYS = ("t", "obj", "slope")   # float outputs (enter, leave, basis, nseg, status: integers)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_parametric_cost_ref())
        L.ref_parametric_cost.restype = C.c_int
        L.ref_parametric_cost.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, _dp, C.c_double,
                                          C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip]
        _lib = L
    return _lib


def parametric_cost(A, b, c, basis, g, t_max=np.inf, maximize=True, eps=1e-9, max_breaks=64):
    """dict(status, nseg, t, obj (max_breaks+2), slope, enter, leave (max_breaks+1), basis (m)), padded with NaN / -1
    past the path (the layout of the batched C calls)."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c, g = (np.ascontiguousarray(v, dtype=np.float64) for v in (b, c, g))
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    nb = max(int(max_breaks), 0)
    t, obj, slope = np.zeros(nb + 2), np.zeros(nb + 2), np.zeros(nb + 1)
    enter, leave = np.zeros(nb + 1, np.int32), np.zeros(nb + 1, np.int32)
    bo, nseg = np.zeros(m, np.int32), C.c_int(-7)
    st = lib().ref_parametric_cost(Af.ctypes.data_as(_dp), m, n, b.ctypes.data_as(_dp), c.ctypes.data_as(_dp),
                                   basis.ctypes.data_as(_ip), int(maximize), g.ctypes.data_as(_dp), float(t_max),
                                   float(eps), int(max_breaks), C.byref(nseg), t.ctypes.data_as(_dp),
                                   obj.ctypes.data_as(_dp), slope.ctypes.data_as(_dp), enter.ctypes.data_as(_ip),
                                   leave.ctypes.data_as(_ip), bo.ctypes.data_as(_ip))
    return dict(status=st, nseg=nseg.value, t=t, obj=obj, slope=slope, enter=enter, leave=leave, basis=bo)


def parametric_cost_batched(A, b, c, basis, g, t_max=np.inf, maximize=True, eps=1e-9, max_breaks=64,
                            run_status=None):
    """The reference per LP with the batched calls' padded layout; LPs whose run_status is not OPTIMAL keep it, get
    nseg 0, NaN / -1 and their basis back (lp_batched_parametric_cost)."""
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
        r = parametric_cost(A[k], b[k], c[k], basis[k], g[k], t_max, maximize, eps, max_breaks)
        for key in out:
            out[key][k] = r[key]
    return out


def trim(r):
    """The single-LP dict of capi.Context.basis_parametric_cost: arrays cut to the path."""
    ns = r["nseg"]
    return dict(status=r["status"], t=r["t"][:ns + 1] if ns else r["t"][:0], obj=r["obj"][:ns + 1] if ns else r["obj"][:0],
                slope=r["slope"][:ns], enter=r["enter"][:ns], leave=r["leave"][:ns], basis=r["basis"])


# ---- cases ---------------------------------------------------------------------------------------------------------

def direction(seed, c, scale=1.0):
    """Seeded cost direction with mixed signs, scaled by |c| (0.5 where c_j = 0)."""
    rng = np.random.default_rng(104729 + seed)
    return rng.uniform(-1.0, 1.0, size=len(c)) * np.where(c != 0.0, np.abs(c), 0.5) * scale


def max_case(seed, m, n):
    """capi.gen_lp (max, bounded) at the oracle's optimal basis with a seeded mixed-sign g: (A, b, c, basis, g,
    maximize).  The path reaches +inf."""
    A, b, c, basis = capi.gen_lp(seed, m, n)
    r = o.simplex_tableau(A, b, c, basis, True, n)
    assert r["status"] == OPTIMAL
    return A, b, c, np.asarray(r["basis"], np.int32), direction(seed, c), True


def min_case(seed, m, k, positive=False):
    """lpcases.min_lp (min over an unbounded region) at the oracle's two-phase optimal basis.  A mixed-sign g ends
    UNBOUNDED once a column with g_j < 0 becomes improving; positive=True (g = |g|) reaches +inf."""
    A, b, c, _ = lpcases.min_lp(seed, m, k)
    r = o.two_phase(A, b, c, False, A.shape[1])
    assert r["status"] == OPTIMAL
    g = direction(seed, c)
    return A, b, c, np.asarray(r["basis"], np.int32), np.abs(g) if positive else g, False


def zero_g_case():
    """capi.gen_lp 8 x 20 with g = 0: one segment of slope 0 and a finite value at +inf."""
    A, b, c, basis, g, mx = max_case(21, 8, 20)
    return A, b, c, basis, np.zeros_like(g), mx


def unbounded_case(maximize=True):
    """max x1 + x2 - 2 y with x1 - y <= 1, x2 <= 3 at its optimum {x1, x2}: y's reduced cost -1 rises with g = e_y
    and reaches 0 at t = 1, where the ray (x1, y) = (1 + s, s) becomes improving: UNBOUNDED at t = 1.  The min
    form is the same LP with c and g negated."""
    A = np.array([[1.0, 0.0, -1.0, 1.0, 0.0],
                  [0.0, 1.0, 0.0, 0.0, 1.0]])
    b = np.array([1.0, 3.0])
    c = np.array([1.0, 1.0, -2.0, 0.0, 0.0])
    g = np.array([0.0, 0.0, 1.0, 0.0, 0.0])
    s = 1.0 if maximize else -1.0
    return A, b, s * c, np.array([0, 1], np.int32), s * g, maximize


def zero_length_case(maximize=True):
    """max x1 + x2 with x1 + u = 1, x2 + v = 1 at {x1, x2} along g = e_u + e_v: u and v both reach reduced cost 0
    at t = 1 on independent rows, so u enters at t = 1 and v at t = 1 again, a segment of length 0.  The min form
    negates c and g."""
    A = np.array([[1.0, 0.0, 1.0, 0.0],
                  [0.0, 1.0, 0.0, 1.0]])
    b = np.array([1.0, 1.0])
    c = np.array([1.0, 1.0, 0.0, 0.0])
    g = np.array([0.0, 0.0, 1.0, 1.0])
    s = 1.0 if maximize else -1.0
    return A, b, s * c, np.array([0, 1], np.int32), s * g, maximize


def named_cases():
    """name -> (A, b, c, basis, g, maximize)."""
    return {
        "max_8x20": max_case(11, 8, 20),
        "max_16x40": max_case(12, 16, 40),
        "max_24x48": max_case(13, 24, 48),
        "min_6x16_inf": min_case(14, 6, 10, positive=True),
        "min_12x32_inf": min_case(15, 12, 20, positive=True),
        "min_12x32_unbounded": min_case(16, 12, 20),
        "zero_g": zero_g_case(),
        "unbounded_max": unbounded_case(True),
        "unbounded_min": unbounded_case(False),
        "zero_length_max": zero_length_case(True),
        "zero_length_min": zero_length_case(False),
    }
