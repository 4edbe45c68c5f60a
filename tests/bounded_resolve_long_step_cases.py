"""The inputs that tests/test_bounded_resolve_long_step_cpu.py and tests/test_gpu_bounded_resolve_long_step.py share, and
their reference results (tests/ref/bounded_resolve_long_step_ref.c through tests/bounded_resolve_long_step_ref.py),
computed once per key and never changed.  A warm start is (A, b, c, lo, hi, basis, at_upper).  Test infrastructure
only."""
import functools

import numpy as np

from tests import bounded_resolve_large_cases as Q
from tests import bounded_resolve_long_step_ref as L

INF = np.inf
OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)

# What the reference counts under Dantzig's dual rule (recorded from tests/ref/bounded_resolve_long_step_ref.c):
# (m, n, seed, maximize, perturbation) -> (iters under the textbook ratio test, iters under the long-step one)
PINNED_ITERS = {(160, 320, 1, True, "bound"): ([41, 0, 0], [28, 0, 27]),
                (160, 320, 6, True, "bound"): ([100, 0, 0], [23, 0, 83]),
                (160, 320, 4, True, "bound"): ([63, 0, 0], [14, 0, 47]),
                (160, 320, 22, False, "bound"): ([214, 0, 0], [72, 0, 127]),   # LP_INFEASIBLE under both
                (200, 500, 1, True, "rhs"): ([56, 0, 0], [19, 0, 49]),
                (64, 192, 1, False, "rhs"): ([29, 0, 0], [12, 0, 15]),
                (32, 96, 1, True, "bound"): ([16, 0, 0], [8, 0, 10]),
                (160, 320, 8, True, "rhs"): ([23, 0, 0], [25, 0, 19])}         # (more pivots than the textbook test)
# the 160 x 320 seed 1 max "bound" case needs 28 dual pivots under the long-step test (41 under the textbook one:
# Q.LIMIT_SWEEP)
LIMIT_SWEEP = {1: ITER_LIMIT, 2: ITER_LIMIT, 27: ITER_LIMIT, 28: ITER_LIMIT, 29: OPTIMAL}
LIMIT_PIVOTS = 28

TALL_MAX_ITER = 12


def _freeze(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(arrays)


def warm(m, n, seed, maximize, kind):
    """The warm start of Q after perturbation `kind` of the m x n LP of `seed`."""
    return Q.warm(m, n, seed, maximize, kind, Q.cold_ref(m, n, seed, maximize))


@functools.lru_cache(maxsize=None)
def tall_boxed(reverse):
    """Q.tall (1100 x 2300, more rows than the selectors have threads) with a box on every structural column: those
    Q.tall leaves unbounded get [0, 0.5].  Its dual loop flips in most iterations, several columns in some, and
    complements rows in most."""
    A, b, c, lo, hi, basis, up = Q.tall(reverse)
    k = A.shape[1] - A.shape[0]
    hi = hi.copy()
    hi[:k] = np.where(np.isinf(hi[:k]), .5, hi[:k])
    return _freeze([A, b, c, lo, hi, basis, up])


@functools.lru_cache(maxsize=None)
def edge(kind):
    """Minimise x0 + 2 x1 + 3 x2 over -x0 - x1 - x2 + s0 = -2, x0 + x1 + x2 + s1 = 10 from the slack basis: row 0 is
    violated below and the entering chain meets x0, x1, x2 in that order (ratios 1, 2, 3).
      "fixed":      hi = (0, inf, inf): x0 is fixed, U = 0, so it is flipped and passed; x1 enters;
      "unbounded":  hi = (1, inf, inf): x0 is flipped (-2 + 1 stays below 0); x1 with U = +inf is pivoted on;
      "cure":       hi = (3, inf, inf): flipping x0 would cure the row (-2 + 3 >= 0), so it is pivoted on, no flip;
      "all":        hi = (.5, .5, .5): every candidate is flipped and -0.5 remains: infeasible, three flags set."""
    A = np.array([[-1., -1., -1., 1., 0.], [1., 1., 1., 0., 1.]])
    b = np.array([-2., 10.])
    c = np.array([1., 2., 3., 0., 0.])
    box = {"fixed": (0., INF, INF), "unbounded": (1., INF, INF), "cure": (3., INF, INF), "all": (.5, .5, .5)}[kind]
    hi = np.array(list(box) + [INF, INF])
    return _freeze([A, b, c, np.zeros(5), hi, np.array([3, 4], np.int32), np.zeros(5, np.int32)])


# kind -> (status, iters, at_upper of the three structural columns)
EDGE_RESULTS = {"fixed": (OPTIMAL, [1, 0, 1], [1, 0, 0]), "unbounded": (OPTIMAL, [1, 0, 1], [1, 0, 0]),
                "cure": (OPTIMAL, [1, 0, 0], [0, 0, 0]), "all": (INFEASIBLE, [0, 0, 3], [1, 1, 1])}


_ref_cache = {}


def ref(key, start, maximize, n_orig=None, eps=1e-9, max_iter=10000, rule=L.DANTZIG, dual_rule=L.DUAL_DANTZIG,
        dual_ratio=L.LONG_STEP):
    """L.resolve(*start, ...), computed once per (key, rule, dual_rule, dual_ratio)."""
    key = (key, rule, dual_rule, dual_ratio)
    if key not in _ref_cache:
        _ref_cache[key] = L.resolve(*start, maximize, n_orig, eps, max_iter, rule, dual_rule, dual_ratio)
    return _ref_cache[key]


def steps(key, start, maximize, upto, dual_rule=L.DUAL_DANTZIG):
    """What each of the first `upto` dual iterations of the long-step re-solve did, read off the reference at
    max_iter = 1 .. upto (an iteration's flips come before its pivot, so they show between max_iter = k - 1 and k): a
    list of dict(flipped: the columns flipped in it, complemented: the leaving variable left at its upper bound,
    before: the result at max_iter = k - 1 or None, after: the result at max_iter = k)."""
    out, prev = [], None
    for k in range(1, upto + 1):
        r = ref((key, "steps", k), start, maximize, max_iter=k, dual_rule=dual_rule)
        if r["status"] != ITER_LIMIT or r["iters"][0] != k:
            break
        b0 = np.asarray(start[5]) if prev is None else prev["basis"]
        u0 = np.asarray(start[6]) if prev is None else prev["at_upper"]
        left = [int(v) for v in b0 if v not in set(r["basis"].tolist())]
        assert len(left) == 1
        changed = set(np.flatnonzero(u0 != r["at_upper"]).tolist())
        flipped = sorted(changed - set(left))
        assert len(flipped) == r["iters"][2] - (0 if prev is None else prev["iters"][2])
        out.append(dict(flipped=flipped, complemented=left[0] in changed, before=prev, after=r))
        prev = r
    return out


def held_row_proves_infeasible(start, result, eps=1e-9, tol=1e-7):
    """In numpy: at the returned basis, with every non-basic column at its flagged bound and every flagged column held
    as U - x, some basis position holds a value below -eps that no non-basic column can raise by moving into its box
    (its entry in that row, in the held signs, is >= -tol; columns with U = 0 cannot move).  tol covers the rounding
    of numpy's solve against the pivoted tableau, orders of magnitude below the entries the ratio test accepts."""
    A, b, _, lo, hi, _, _ = start
    basis, up = np.asarray(result["basis"]), np.asarray(result["at_upper"])
    m, n = A.shape
    U = hi - lo
    non = np.setdiff1d(np.arange(n), basis)
    rhs = b - A @ lo
    for j in non:
        if up[j]:
            rhs = rhs - A[:, j] * U[j]
    Binv = np.linalg.inv(A[:, basis])
    xB = Binv @ rhs
    rows = Binv @ A[:, non]
    sign_j = np.where(up[non] != 0, -1., 1.)
    movable = U[non] > 0
    for t in range(m):
        k = basis[t]
        held = U[k] - xB[t] if up[k] else xB[t]
        if not held < -eps:
            continue
        entries = (-1. if up[k] else 1.) * sign_j * rows[t]
        if np.all(entries[movable] >= -tol):
            return True
    return False
