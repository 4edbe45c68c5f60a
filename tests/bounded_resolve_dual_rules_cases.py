"""The inputs that tests/test_bounded_resolve_dual_rules_cpu.py and tests/test_gpu_bounded_resolve_dual_rules.py share,
and their reference results (tests/ref/bounded_resolve_dual_rules_ref.c through tests/bounded_resolve_dual_rules_ref.py),
computed once per key and never changed.  A warm start is (A, b, c, lo, hi, basis, at_upper).  Test infrastructure
only."""
import functools

import numpy as np

from tests import bounded_resolve_dual_rules_ref as D
from tests import bounded_resolve_large_cases as Q

INF = np.inf
OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)

# The reference's dual pivot counts under DUAL_DEVEX (recorded from tests/ref/bounded_resolve_dual_rules_ref.c):
# (m, n, seed, maximize, perturbation) -> iters
DEVEX_ITERS = {(160, 320, 1, True, "bound"): [47, 0, 0], (160, 320, 1, True, "rhs"): [25, 0, 0],
               (160, 320, 2, False, "bound"): [48, 0, 0]}
# the 160 x 320 seed 1 max "bound" case needs 47 dual pivots under Devex (41 under Dantzig: Q.LIMIT_SWEEP)
DEVEX_LIMIT_SWEEP = {1: ITER_LIMIT, 2: ITER_LIMIT, 46: ITER_LIMIT, 47: ITER_LIMIT, 48: OPTIMAL}
DEVEX_LIMIT_PIVOTS = 47

# Q.tall under Devex at Q.TALL_MAX_ITER: still short of its verdict; the flags set by then
TALL_DEVEX_ITERS = [60, 0, 0]
TALL_DEVEX_FLAGS = 27


def _freeze(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def tie(m, n, p, seed=11):
    """A minimisation from the slack basis in order (no crash; xB = b) whose positions p and p + 1 carry the same most
    negative b, -2.0; every other b lies in [-1, 2), so every other violation is strictly smaller in magnitude.  With
    every weight 1.0 the two tie exactly on v * v / w and position p must leave.  lo = 0, some columns boxed, as
    Q.tall."""
    assert 0 <= p < m - 1 and n > m
    rng = np.random.default_rng(seed)
    k = n - m
    A = np.hstack([rng.uniform(-1, 1, (m, k)).round(2), np.eye(m)])
    c = np.concatenate([rng.uniform(.1, 1, k).round(2), np.zeros(m)])
    b = rng.uniform(-1, 2, m).round(2)
    b[p] = b[p + 1] = -2.0
    lo, hi = np.zeros(n), np.full(n, INF)
    hi[k:] = np.where(rng.random(m) < .5, .5, INF)
    hi[:k] = np.where(rng.random(k) < .5, 1., INF)
    return _freeze([A, b, c, lo, hi, np.arange(k, n, dtype=np.int32), np.zeros(n, np.int32)])


TIE_SMALL = (67, 201, 63)       # the last position of the first wave against the first of the second (fits LDS)
TIE_LARGE = (1100, 2300, 1023)  # the last position of the selector's first pass against the first of its second


def left_at(start, result):
    """The basis positions whose variable differs between a warm start and a result."""
    return np.flatnonzero(np.asarray(start[5]) != np.asarray(result["basis"])).tolist()


_ref_cache = {}


def ref(key, start, maximize, n_orig=None, eps=1e-9, max_iter=10000, rule=D.DANTZIG, dual_rule=D.DUAL_DEVEX):
    """D.resolve(*start, ...), computed once per (key, rule, dual_rule)."""
    key = (key, rule, dual_rule)
    if key not in _ref_cache:
        _ref_cache[key] = D.resolve(*start, maximize, n_orig, eps, max_iter, rule, dual_rule)
    return _ref_cache[key]


def warm_160(seed, maximize, kind):
    """The warm start of Q after perturbation `kind` of the 160 x 320 LP of `seed`."""
    return Q.warm(160, 320, seed, maximize, kind, Q.cold_ref(160, 320, seed, maximize))
