"""The inputs that tests/test_bounded_resolve_large_cpu.py and tests/test_gpu_bounded_resolve_large.py share, and their
reference results (tests/ref/bounded_resolve_ref.c through tests/bounded_resolve_ref.py), computed once per key and
never changed.  A warm start is (A, b, c, lo, hi, basis, at_upper).  Test infrastructure only."""
import functools

import numpy as np

from tests import bounded_large_cases as K
from tests import bounded_resolve_ref as W

INF = np.inf
OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)

LDS_SHAPES = [(6, 16), (32, 96), (64, 192)]
LDS_SEEDS = (1, 2, 3)
# bounded_ref.boxed_lp(seed, m, n, maximize, "mixed") beyond lp_simplex_bounded_fits; 67 x 201 still fits and is here for
# its odd row length (202 columns padded to 208)
BEYOND = [(160, 320, s) for s in range(1, 9)] + [(200, 500, 1)] + [(67, 201, s) for s in (1, 2)]
# what the reference counts on some of them: (m, n, seed, maximize, perturbation) -> iters
BEYOND_ITERS = {(160, 320, 1, True, "bound"): [41, 0, 0], (160, 320, 1, True, "cost"): [0, 15, 3],
                (160, 320, 1, True, "rhs"): [33, 0, 0]}
# LP_INFEASIBLE from the dual loop with consistent bounds: 160 x 320, "bound", (seed, maximize) -> iters where pinned
DUAL_INFEASIBLE = [(s, mx) for s in (20, 22, 33) for mx in (True, False)]
DUAL_INFEASIBLE_ITERS = {(22, True): [28, 0, 0], (20, True): [112, 0, 0]}
# the 160 x 320 seed 1 max "bound" case needs 41 dual pivots
LIMIT_SWEEP = {1: ITER_LIMIT, 2: ITER_LIMIT, 40: ITER_LIMIT, 41: ITER_LIMIT, 42: OPTIMAL}

TALL_SHAPE = (1100, 2300)
TALL_MAX_ITER = 60
TALL_ITERS = [60, 0, 0]
TALL_FLAGS = 35

UNIT_COST_ITERS = {(1, False): [0, 423, 0], (1, True): [0, 379, 0]}


def _freeze(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(arrays)


def cold_ref(m, n, seed, maximize):
    """The reference's cold solve of K.boxed(m, n, "mixed", seed, maximize) with the full x: what lp_simplex_bounded
    and lp_simplex_bounded_large return bit for bit."""
    A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, maximize)
    return K.ref(("resolve-large-cold", m, n, seed, maximize), A, b, c, lo, hi, maximize)


def warm(m, n, seed, maximize, kind, cold):
    """The warm start after perturbation `kind` of K.boxed(m, n, "mixed", seed, maximize), from the optimal cold result
    `cold` (with the full x)."""
    A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, maximize)
    b2, c2, lo2, hi2 = W.perturb(seed, kind, b, c, lo, hi, cold["basis"], cold["x"])
    return A, b2, c2, lo2, hi2, cold["basis"], cold["at_upper"]


def outcomes_160(cold, maximize=True, seed=1, limit=5):
    """One warm start per outcome the perturbed 160 x 320 cases do not reach, by the constructions of
    bounded_resolve_ref.outcome_cases: a list of (name, warm start, status, max_iter)."""
    m, n = 160, 320
    A, b, c, lo, hi, _ = K.boxed(m, n, "mixed", seed, maximize)
    basis, up = cold["basis"], cold["at_upper"]
    out = []
    hi2 = hi.copy()
    hi2[seed % n] = lo[seed % n] - 0.5
    out.append(("crossed", (A, b, c, lo, hi2, basis, up), INFEASIBLE, 10000))
    # (lo_j = 0: zeroing the column leaves the shifted right-hand side, and with it the primal feasible start, alone)
    free = [j for j in range(n) if j not in set(basis.tolist()) and np.isinf(hi[j]) and not up[j] and lo[j] == 0.0]
    A2, c2 = A.copy(), c.copy()
    A2[:, free[0]] = 0.0
    c2[free[0]] = 1.0 if maximize else -1.0
    out.append(("unbounded", (A2, b, c2, lo, hi, basis, up), UNBOUNDED, 10000))
    twice = basis.copy()
    twice[1] = twice[0]
    out.append(("singular", (A, b, c, lo, hi, twice, up), SINGULAR, 10000))
    b2, _, _, _ = W.perturb(seed, "rhs", b, c, lo, hi, basis, cold["x"])
    _, c2, _, _ = W.perturb(seed, "cost", b, c, lo, hi, basis, cold["x"])
    out.append(("no_valid_start", (A, b2, c2, lo, hi, basis, up), BAD_ARG, 10000))
    out.append(("iter_limit", warm(m, n, seed, maximize, "bound", cold), ITER_LIMIT, limit))
    return out


@functools.lru_cache(maxsize=None)
def tall(reverse):
    """More rows than the selectors have threads: a minimisation from the slack basis (in order: the crash is skipped;
    reversed: the crash and the row permutation run) whose dual loop complements rows."""
    m, n = TALL_SHAPE
    rng = np.random.default_rng(5)
    k = n - m
    A = np.hstack([rng.uniform(-1, 1, (m, k)).round(2), np.eye(m)])
    c = np.concatenate([rng.uniform(.1, 1, k).round(2), np.zeros(m)])
    b = rng.uniform(-1, 2, m).round(2)
    lo, hi = np.zeros(n), np.full(n, INF)
    hi[k:] = np.where(rng.random(m) < .5, .5, INF)
    hi[:k] = np.where(rng.random(k) < .5, 1., INF)
    basis = np.arange(k, n, dtype=np.int32)
    if reverse:
        basis = basis[::-1].copy()
    return _freeze([A, b, c, lo, hi, basis, np.zeros(n, np.int32)])


@functools.lru_cache(maxsize=None)
def unit_costs(seed, reverse):
    """160 x 320 from the slack basis (in order or reversed) with non-zero slack costs, lo = 0, hi = inf: the basis
    install has costs to price out over a unit basis.  b >= 0, so the start is primal feasible and the primal loop
    runs, to OPTIMAL in both senses."""
    m, n = 160, 320
    rng = np.random.default_rng(seed)
    k = n - m
    A = np.hstack([rng.uniform(-1, 1, (m, k)).round(2), np.eye(m)])
    c = np.concatenate([rng.uniform(-1, 1, k).round(2), rng.uniform(.1, .5, m).round(2)])
    b = rng.uniform(0, .4, m).round(2)
    lo, hi = np.zeros(n), np.full(n, INF)
    basis = np.arange(k, n, dtype=np.int32)
    if reverse:
        basis = basis[::-1].copy()
    return _freeze([A, b, c, lo, hi, basis, np.zeros(n, np.int32)])


_ref_cache = {}


def ref(key, start, maximize, n_orig=None, eps=1e-9, max_iter=10000):
    """W.resolve(*start, ...), computed once per key."""
    if key not in _ref_cache:
        _ref_cache[key] = W.resolve(*start, maximize, n_orig, eps, max_iter)
    return _ref_cache[key]
