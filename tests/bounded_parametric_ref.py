"""ctypes binding of tests/ref/bounded_parametric_ref.c (the parametric right-hand-side path b + t d and the parametric
cost path c + t g of a bounded-variable LP from an optimal basis and its at-upper flags) and the cases the CPU, GPU and
C++ tests share.  Test infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build
from tests import bounded_ref as B
from tests import parametric_cost_ref as PC
from tests import parametric_ref as PR

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
KEYS = ("status", "nseg", "t", "obj", "slope", "enter", "leave", "side", "basis", "at_upper")
PATHS = ("rhs", "cost")


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_bounded_parametric_ref())
        for fn in (L.ref_bounded_parametric, L.ref_bounded_parametric_cost):
            fn.restype = C.c_int
            fn.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, _dp, C.c_double, C.c_double,
                           C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip, _ip, _ip]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def parametric(path, A, b, c, lo, hi, basis, at_upper, direction, t_max=np.inf, maximize=True, eps=1e-9,
               max_breaks=64):
    """path "rhs": direction = d (m); "cost": direction = g (n).  dict(status, nseg, t, obj (max_breaks+2), slope,
    enter, leave, side (max_breaks+1), basis (m), at_upper (n)), padded with NaN / -1 past the path (the layout of the
    batched C calls)."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c, lo, hi, direction = (np.ascontiguousarray(v, dtype=np.float64) for v in (b, c, lo, hi, direction))
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    at_upper = np.ascontiguousarray(at_upper, dtype=np.int32)
    assert basis.shape == (m,) and at_upper.shape == (n,) and direction.shape == ((m,) if path == "rhs" else (n,))
    nb = max(int(max_breaks), 0)
    t, obj, slope = np.zeros(nb + 2), np.zeros(nb + 2), np.zeros(nb + 1)
    enter, leave, side = (np.zeros(nb + 1, np.int32) for _ in range(3))
    bo, uo, nseg = np.zeros(m, np.int32), np.zeros(n, np.int32), C.c_int(-7)
    fn = lib().ref_bounded_parametric if path == "rhs" else lib().ref_bounded_parametric_cost
    st = fn(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize), _d(direction),
            float(t_max), float(eps), int(max_breaks), C.byref(nseg), _d(t), _d(obj), _d(slope), _i(enter), _i(leave),
            _i(side), _i(bo), _i(uo))
    return dict(status=st, nseg=nseg.value, t=t, obj=obj, slope=slope, enter=enter, leave=leave, side=side, basis=bo,
                at_upper=uo)


def parametric_batched(path, A, b, c, lo, hi, basis, at_upper, direction, t_max=np.inf, maximize=True, eps=1e-9,
                       max_breaks=64, run_status=None):
    """The reference per LP with the batched calls' padded layout; LPs whose run_status is not OPTIMAL keep it, get
    nseg 0, NaN / -1 and their basis and flags back."""
    batch, m, n = np.shape(A)
    nb = int(max_breaks)
    out = dict(status=np.zeros(batch, np.int32), nseg=np.zeros(batch, np.int32), t=np.full((batch, nb + 2), np.nan),
               obj=np.full((batch, nb + 2), np.nan), slope=np.full((batch, nb + 1), np.nan),
               enter=np.full((batch, nb + 1), -1, np.int32), leave=np.full((batch, nb + 1), -1, np.int32),
               side=np.full((batch, nb + 1), -1, np.int32), basis=np.array(basis, dtype=np.int32).reshape(batch, m),
               at_upper=np.array(at_upper, dtype=np.int32).reshape(batch, n))
    for k in range(batch):
        if run_status is not None and run_status[k] != OPTIMAL:
            out["status"][k] = run_status[k]
            continue
        r = parametric(path, A[k], b[k], c[k], lo[k], hi[k], basis[k], at_upper[k], direction[k], t_max, maximize, eps,
                       max_breaks)
        for key in out:
            out[key][k] = r[key]
    return out


def trim(r):
    """The single-LP dict of capi.Context.bounded_parametric / bounded_parametric_cost: arrays cut to the path."""
    ns = r["nseg"]
    return dict(status=r["status"], t=r["t"][:ns + 1] if ns else r["t"][:0], obj=r["obj"][:ns + 1] if ns else r["obj"][:0],
                slope=r["slope"][:ns], enter=r["enter"][:ns], leave=r["leave"][:ns], side=r["side"][:ns],
                basis=r["basis"], at_upper=r["at_upper"])


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, keys=None):
    """Every key of `want` (or `keys`) equals `got` bit for bit (floats: NaN where NaN, signed zeros included)."""
    for k in (keys or want.keys()):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if w.dtype.kind == "f":
            assert np.array_equal(bits(g), bits(w)), k
        else:
            assert np.array_equal(g, w), k


# ---- cases ---------------------------------------------------------------------------------------------------------

def boxed_case(path, seed, m, n, maximize=None, kind="mixed"):
    """bounded_ref.boxed_lp at the reference's optimum with a seeded direction (mixed signs, scaled by |b| or |c|):
    (A, b, c, lo, hi, basis, at_upper, direction, maximize), or None when the cold solve is not optimal.  kind "ray"
    (cost path): boxed_lp's "unbounded" column (no row entry, no upper bound) with its cost turned against the sense,
    and a direction that turns it back at t = 1/2, so that the path ends UNBOUNDED."""
    A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n, maximize, "unbounded" if kind == "ray" else kind)
    rng = np.random.default_rng(104729 + seed)
    if path == "rhs":
        direction = rng.uniform(-1.0, 1.0, m) * np.abs(b)
    else:
        direction = rng.uniform(-1.0, 1.0, n) * (np.abs(c) + 0.25)
    if kind == "ray":
        j = int(np.flatnonzero(~A.any(axis=0))[0])
        c[j] = -c[j]
        if path == "cost":
            direction[j] = -2.0 * c[j]
    r = B.bounded(A, b, c, lo, hi, mx)
    if r["status"] != OPTIMAL:
        return None
    return A, b, c, lo, hi, r["basis"], r["at_upper"], direction, mx


def random_cases(path, m, n, count, first_seed=1, maximize=None):
    """`count` boxed cases of one shape, of one sense or (maximize None) both in turn, every fifth of kind "ray", skipping
    seeds whose cold solve is not optimal."""
    out, seed = [], first_seed
    while len(out) < count:
        mx = bool(len(out) % 2) if maximize is None else maximize
        case = boxed_case(path, seed, m, n, mx, "ray" if len(out) % 5 == 4 else "mixed")
        seed += 1
        if case is not None:
            out.append(case)
    return out


def stack(cases):
    """A list of cases of one shape and sense -> the batched arrays (A, b, c, lo, hi, basis, at_upper, direction)."""
    return tuple(np.stack([cs[i] for cs in cases]) for i in range(8))


def plain_as_boxed(case):
    """A case of parametric_ref / parametric_cost_ref (A, b, c, basis, direction, maximize) with lo = 0, hi = inf and
    no flag."""
    A, b, c, basis, direction, mx = case
    n = A.shape[1]
    return A, b, c, np.zeros(n), np.full(n, np.inf), basis, np.zeros(n, np.int32), direction, mx


def _small():
    """max x0 + 2 x1 + 0 x2 with x0 + x1 + s0 = 4, x0 - x1 + s1 = 2 (+ x2 in row 1), 0 <= x0 <= 3, 0 <= x1 <= 2.5,
    x2 fixed at 1: optimum x0 = 1.5, x1 = 2.5 (at its upper bound), s1 basic."""
    A = np.array([[1.0, 1.0, 0.0, 1.0, 0.0],
                  [1.0, -1.0, 1.0, 0.0, 1.0]])
    b = np.array([4.0, 2.0])
    c = np.array([1.0, 2.0, 0.0, 0.0, 0.0])
    lo = np.array([0.0, 0.0, 1.0, 0.0, 0.0])
    hi = np.array([3.0, 2.5, 1.0, np.inf, np.inf])
    return A, b, c, lo, hi


def _at_optimum(A, b, c, lo, hi, maximize):
    r = B.bounded(A, b, c, lo, hi, maximize)
    assert r["status"] == OPTIMAL
    return r["basis"], r["at_upper"]


def _first(path, m, n, pred):
    """The first random case of one shape whose full path satisfies pred."""
    for case in random_cases(path, m, n, 60):
        if pred(case, parametric(path, *case[:8], maximize=case[8])):
            return case
    raise AssertionError("no such case among the first 60")


def named_cases():
    """name -> (path, (A, b, c, lo, hi, basis, at_upper, direction, maximize), kwargs of parametric(), status)."""
    cases = {}
    A, b, c, lo, hi = _small()
    basis, up = _at_optimum(A, b, c, lo, hi, True)
    # b0 grows: x0 = 1.5 + t reaches its upper bound 3 at t = 1.5
    cases["rhs_upper_blocked"] = ("rhs", (A, b, c, lo, hi, basis, up, np.array([1.0, 0.0]), True), {}, None)
    cases["rhs_tmax_inside"] = ("rhs", (A, b, c, lo, hi, basis, up, np.array([1.0, 0.0]), True), dict(t_max=0.75),
                                OPTIMAL)
    cases["rhs_iter_limit"] = ("rhs", (A, b, c, lo, hi, basis, up, np.array([1.0, 0.0]), True), dict(max_breaks=0),
                               ITER_LIMIT)
    # b0 shrinks below what lo allows: infeasible past the last breakpoint
    cases["rhs_infeasible_end"] = ("rhs", (A, b, c, lo, hi, basis, up, np.array([-1.0, 0.0]), True), {}, INFEASIBLE)
    # only the free slack's row moves: feasible for every t
    cases["rhs_end_at_inf"] = ("rhs", (A, b, c, lo, hi, basis, up, np.array([0.0, 1.0]), True), {}, OPTIMAL)
    # cost: x1's cost falls until it leaves its upper bound; x0's rises
    cases["cost_fixed_flip"] = ("cost", (A, b, c, lo, hi, basis, up, np.array([0.0, -1.0, 0.0, 0.0, 0.0]), True), {},
                                None)
    # the first random 6 x 14 case with a bound flip of a column of positive width at t > 0
    cases["cost_flip"] = ("cost", _first("cost", 6, 14, lambda case, r: any(
        e == l and e >= 0 and case[4][e] > case[3][e] and t > 0
        for e, l, t in zip(r["enter"], r["leave"], r["t"][1:]))), {}, None)
    # the first random 6 x 14 case with a pivot (not a flip) whose leaving variable stops at its upper bound at t > 0
    cases["cost_leave_at_upper"] = ("cost", _first("cost", 6, 14, lambda case, r: (
        (r["enter"] != r["leave"]) & (r["leave"] >= 0) & (r["side"] == 1) & (r["t"][1:] > 0)).any()), {}, None)
    cases["cost_tmax_inside"] = ("cost", (A, b, c, lo, hi, basis, up, np.array([0.0, -1.0, 0.0, 0.0, 0.0]), True),
                                 dict(t_max=0.75), OPTIMAL)
    cases["cost_iter_limit"] = ("cost", (A, b, c, lo, hi, basis, up, np.array([0.0, -1.0, 0.0, 0.0, 0.0]), True),
                                dict(max_breaks=0), ITER_LIMIT)
    # a column without an upper bound and without a row entry gets an improving cost at t = 1
    Au = np.hstack([A, np.zeros((2, 1))])
    cu, lou, hiu = np.append(c, -1.0), np.append(lo, 0.0), np.append(hi, np.inf)
    bu, uu = _at_optimum(Au, b, cu, lou, hiu, True)
    cases["cost_unbounded_end"] = ("cost", (Au, b, cu, lou, hiu, bu, uu, np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0]), True),
                                   {}, UNBOUNDED)
    cases["cost_end_at_inf"] = ("cost", (A, b, c, lo, hi, basis, up, np.array([1.0, 1.0, 0.0, 0.0, 0.0]), True), {},
                                OPTIMAL)
    # the plain family's zero-length segment, boxed loosely so that no bound interferes
    Az, bz, cz, basz, dz, mxz = PR.zero_length_case()
    nz = Az.shape[1]
    cases["rhs_zero_length"] = ("rhs", (Az, bz, cz, np.zeros(nz), np.full(nz, 100.0), basz, np.zeros(nz, np.int32), dz,
                                        mxz), {}, None)
    # a fixed column (lo = hi) in the basis: degenerate, U = 0
    Af = np.array([[1.0, 1.0, 1.0, 0.0],
                   [1.0, -1.0, 0.0, 1.0]])
    bf, cf = np.array([3.0, 1.0]), np.array([1.0, 1.0, 0.0, 0.0])
    lof, hif = np.array([0.0, 1.0, 0.0, 0.0]), np.array([5.0, 1.0, np.inf, np.inf])
    cases["rhs_fixed_basic"] = ("rhs", (Af, bf, cf, lof, hif, np.array([0, 1], np.int32), np.zeros(4, np.int32),
                                        np.array([1.0, 0.5]), True), {}, None)
    cases["cost_fixed_basic"] = ("cost", (Af, bf, cf, lof, hif, np.array([0, 1], np.int32), np.zeros(4, np.int32),
                                          np.array([-1.0, 0.0, 0.0, 0.0]), True), {}, None)
    # no path
    hx = hi.copy()
    hx[0] = -1.0
    cases["crossed"] = ("rhs", (A, b, c, lo, hx, basis, up, np.array([1.0, 0.0]), True), {}, INFEASIBLE)
    cases["cost_crossed"] = ("cost", (A, b, c, lo, hx, basis, up, np.zeros(5), True), {}, INFEASIBLE)
    cases["singular"] = ("rhs", (A, b, c, lo, hi, np.array([3, 3], np.int32), np.zeros(5, np.int32),
                                 np.array([1.0, 0.0]), True), {}, SINGULAR)
    cases["cost_singular"] = ("cost", (A, b, c, lo, hi, np.array([0, 0], np.int32), np.zeros(5, np.int32), np.zeros(5),
                                       True), {}, SINGULAR)
    # the slack basis is primal feasible but not dual feasible for max; for b < 0 it is not primal feasible
    cases["start_dual_infeasible"] = ("rhs", (A, b, c, lo, hi, np.array([3, 4], np.int32), np.zeros(5, np.int32),
                                              np.array([1.0, 0.0]), True), {}, BAD_ARG)
    cases["start_primal_infeasible"] = ("cost", (A, -b, -c, lo, hi, np.array([3, 4], np.int32), np.zeros(5, np.int32),
                                                 np.zeros(5), True), {}, BAD_ARG)
    return cases


def plain_named_cases():
    """The named cases of parametric_ref ("rhs") and parametric_cost_ref ("cost") as boxed cases with lo = 0, hi = inf:
    a list of (path, name, plain case, boxed case)."""
    out = [("rhs", name, case, plain_as_boxed(case)) for name, case in PR.named_cases().items()]
    out += [("cost", name, case, plain_as_boxed(case)) for name, case in PC.named_cases().items()]
    return out
