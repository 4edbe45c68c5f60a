"""ctypes binding of tests/ref/bounded_resolve_ref.c (the bounded-variable re-solve from a given basis and given
complement flags) and the perturbations the bounded re-solve tests and scripts/time_bounded_resolve.py share.  Test
infrastructure only."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build
from tests import bounded_ref as B

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build.build_bounded_resolve_ref())
        L.ref_bounded_resolve.restype = C.c_int
        L.ref_bounded_resolve.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int,
                                          C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def resolve(A, b, c, lo, hi, basis, at_upper, maximize=False, n_orig=None, eps=1e-9, max_iter=10000):
    """dict(status, x (n_orig, NaN unless optimal), basis, at_upper, obj (NaN unless optimal), iters (dual pivots,
    primal pivots, bound flips))."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    n_orig = n if n_orig is None else int(n_orig)
    Af = np.ascontiguousarray(A.T).reshape(-1)
    b, c = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    basis = np.ascontiguousarray(basis, dtype=np.int32)
    at_upper = np.ascontiguousarray(at_upper, dtype=np.int32)
    assert basis.shape == (m,) and at_upper.shape == (n,)
    x = np.full(n_orig, np.nan)
    bo = np.full(m, -1, dtype=np.int32)
    up = np.zeros(n, dtype=np.int32)
    obj = C.c_double(float("nan"))
    it = np.zeros(3, dtype=np.int32)
    st = lib().ref_bounded_resolve(_d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize),
                                   n_orig, eps, max_iter, _d(x), _i(bo), _i(up), C.byref(obj), _i(it))
    return dict(status=st, x=x, basis=bo, at_upper=up, obj=obj.value, iters=it.tolist())


PERTURBATIONS = ("bound", "rhs", "cost")


def perturb(seed, kind, b, c, lo, hi, basis, x):
    """(b', c', lo', hi') for an LP whose cold solve was optimal with `basis` and the full vertex x (n), seeded by
    default_rng(1000 + seed).  kind:
      "bound"  one to three basic columns (slacks included) get, with equal chance, hi pulled to lo + (x - lo) u,
               u in [0.2, 0.9], or lo pushed to x + (top - x) u, u in [0.1, 0.8], top = hi, or x + 1 for an infinite
               hi: a branch, a fixing, a what-if.  The old basis stays dual feasible;
      "rhs"    one to three rows of b scaled by [0.3, 0.9];
      "cost"   three costs moved by up to 0.5 either way: the old basis stays primal feasible."""
    rng = np.random.default_rng(1000 + seed)
    b2, c2, lo2, hi2 = (np.array(v, dtype=np.float64) for v in (b, c, lo, hi))
    n = len(c2)
    assert len(x) == n
    if kind == "bound":
        cand = [int(k) for k in basis]
        for k in rng.choice(cand, size=min(len(cand), int(rng.integers(1, 4))), replace=False):
            if rng.random() < 0.5:
                hi2[k] = lo2[k] + (x[k] - lo2[k]) * rng.uniform(0.2, 0.9)
            else:
                top = hi2[k] if np.isfinite(hi2[k]) else x[k] + 1.0
                lo2[k] = x[k] + (top - x[k]) * rng.uniform(0.1, 0.8)
    elif kind == "rhs":
        for i in rng.choice(len(b2), size=min(len(b2), int(rng.integers(1, 4))), replace=False):
            b2[i] *= rng.uniform(0.3, 0.9)
    elif kind == "cost":
        for j in rng.choice(n, size=3, replace=False):
            c2[j] += rng.uniform(-0.5, 0.5)
    else:
        raise ValueError(kind)
    return b2, c2, lo2, hi2


def outcome_cases(m=6, n=16, max_iter=3, maximize=True, seeds=400):
    """One warm start per outcome of the re-solve under one max_iter, found by the reference on
    bounded_ref.boxed_lp(seed, m, n, kind="mixed"): a list of (name, (A, b, c, lo, hi, basis, at_upper), status).
      dual_complement   optimal by the dual loop with a position complemented first (a flag differs, no flip)
      primal_flip       optimal by the primal loop with at least one bound flip
      dual_infeasible   INFEASIBLE from the dual loop (consistent bounds)
      crossed           one hi pulled below its lo
      unbounded         a non-basic column with infinite hi gets a zero A column and an improving cost
      iter_limit        more dual pivots needed than max_iter
      singular          a repeated basis column
      no_valid_start    b and c both changed: neither primal nor dual feasible, the per-LP BAD_ARG"""
    def cold(seed):
        A, b, c, lo, hi, _ = B.boxed_lp(seed, m, n, maximize=maximize, kind="mixed")
        r = B.bounded(A, b, c, lo, hi, maximize)
        return (A, b, c, lo, hi, r) if r["status"] == OPTIMAL else None

    def run(A, b, c, lo, hi, basis, up):
        return resolve(A, b, c, lo, hi, basis, up, maximize, max_iter=max_iter)

    def bound(seed):
        A, b, c, lo, hi, r = cold(seed)
        _, _, lo2, hi2 = perturb(seed, "bound", b, c, lo, hi, r["basis"], r["x"])
        return A, b, c, lo2, hi2, r["basis"], r["at_upper"]

    def dual_complement(seed):
        cs = bound(seed)
        g = run(*cs)
        return cs if (g["status"] == OPTIMAL and g["iters"][0] > 0 and g["iters"][2] == 0
                      and np.any(g["at_upper"] != cs[6])) else None

    def primal_flip(seed):
        A, b, c, lo, hi, r = cold(seed)
        _, c2, _, _ = perturb(seed, "cost", b, c, lo, hi, r["basis"], r["x"])
        cs = (A, b, c2, lo, hi, r["basis"], r["at_upper"])
        g = run(*cs)
        return cs if g["status"] == OPTIMAL and g["iters"][0] == 0 and g["iters"][2] > 0 else None

    def dual_infeasible(seed):
        cs = bound(seed)
        g = run(*cs)
        return cs if g["status"] == INFEASIBLE and not np.any(cs[4] < cs[3]) else None

    def crossed(seed):
        A, b, c, lo, hi, r = cold(seed)
        hi2 = hi.copy()
        hi2[seed % n] = lo[seed % n] - 0.5
        return A, b, c, lo, hi2, r["basis"], r["at_upper"]

    def unbounded(seed):
        A, b, c, lo, hi, r = cold(seed)
        free = [j for j in range(n) if j not in set(r["basis"].tolist()) and np.isinf(hi[j]) and not r["at_upper"][j]]
        if not free:
            return None
        A2, c2 = A.copy(), c.copy()
        A2[:, free[0]] = 0.0
        c2[free[0]] = 1.0 if maximize else -1.0
        cs = (A2, b, c2, lo, hi, r["basis"], r["at_upper"])
        return cs if run(*cs)["status"] == UNBOUNDED else None

    def iter_limit(seed):
        cs = bound(seed)
        g = run(*cs)
        return cs if g["status"] == ITER_LIMIT and g["iters"] == [max_iter, 0, 0] else None

    def singular(seed):
        A, b, c, lo, hi, r = cold(seed)
        basis = r["basis"].copy()
        basis[1] = basis[0]
        cs = (A, b, c, lo, hi, basis, r["at_upper"])
        return cs if run(*cs)["status"] == SINGULAR else None

    def no_valid_start(seed):
        A, b, c, lo, hi, r = cold(seed)
        b2, _, _, _ = perturb(seed, "rhs", b, c, lo, hi, r["basis"], r["x"])
        _, c2, _, _ = perturb(seed, "cost", b, c, lo, hi, r["basis"], r["x"])
        cs = (A, b2, c2, lo, hi, r["basis"], r["at_upper"])
        return cs if run(*cs)["status"] == BAD_ARG else None

    want = [(dual_complement, OPTIMAL), (primal_flip, OPTIMAL), (dual_infeasible, INFEASIBLE), (crossed, INFEASIBLE),
            (unbounded, UNBOUNDED), (iter_limit, ITER_LIMIT), (singular, SINGULAR), (no_valid_start, BAD_ARG)]
    picked = []
    for find, status in want:
        for seed in range(seeds):
            if cold(seed) is None:
                continue
            cs = find(seed)
            if cs is not None:
                picked.append((find.__name__, cs, status))
                break
        else:
            raise AssertionError(f"no {find.__name__} case under max_iter = {max_iter}")
    return picked
