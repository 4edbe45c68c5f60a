"""The inputs that tests/test_bounded_large_cpu.py and tests/test_gpu_bounded_large.py share, and their reference results
(tests/ref/bounded_ref.c through tests/bounded_ref.py), computed once per process and never changed.  Test
infrastructure only."""
import functools

import numpy as np

from tests import bounded_ref as R
from tests import lpcases

INF = np.inf

# (m, n, kind, seed) of bounded_ref.boxed_lp beyond lp_simplex_bounded_fits, with what the reference returns there:
# status, iters (phase-I pivots, drive-out pivots, phase-II pivots, flips)
BEYOND = {
    (160, 320, "mixed", 1): (R.OPTIMAL, [930, 0, 208, 475]),
    (160, 320, "box", 1): (R.OPTIMAL, [782, 0, 130, 99]),
    (160, 320, "unbounded", 1): (R.UNBOUNDED, [915, 0, 74, 430]),
    (160, 320, "infeasible", 1): (R.INFEASIBLE, None),
    (160, 320, "crossed", 1): (R.INFEASIBLE, [0, 0, 0, 0]),
    (200, 500, "mixed", 1): (R.OPTIMAL, [2199, 0, 660, 1389]),
}
BEYOND_CASES = ([(67, 201, "mixed", s) for s in (1, 2)]
                + [(160, 320, kind, s) for kind in ("mixed", "box", "unbounded", "infeasible", "crossed") for s in (1, 2)]
                + [(200, 500, "mixed", 1)])

# more rows than the selector has threads, max_iter = 150: (kind, seed) -> iters at the iteration limit
TALL = {("mixed", 1): [100, 0, 0, 50], ("mixed", 2): [92, 0, 0, 58], ("box", 1): [0, 0, 0, 150]}
TALL_SHAPE = (1100, 2300)
TALL_MAX_ITER = 150

SINGULAR_FLIPS = {1: 417, 2: 360, 3: 250}
DRIVEOUT_PIVOTS = {5: 5, 6: 5, 7: 4, 8: 4}


@functools.lru_cache(maxsize=None)
def boxed(m, n, kind, seed, maximize=None):
    """(A, b, c, lo, hi, maximize) of bounded_ref.boxed_lp; the arrays are read-only."""
    case = R.boxed_lp(seed, m, n, maximize, kind)
    for a in case[:5]:
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def singular(seed):
    """boxed_lp(seed, 160, 320, "mixed") with row m-1 replaced by row 0, b likewise: dependent rows."""
    A, b, c, lo, hi, mx = R.boxed_lp(seed, 160, 320, kind="mixed")
    A[-1] = A[0]
    b[-1] = b[0]
    return A, b, c, lo, hi, mx


@functools.lru_cache(maxsize=None)
def driveout(seed):
    """lpcases.degenerate_eq_lp(seed, 40, 70, 20) with half of the columns boxed to [0, 2]: phase I ends with
    artificials basic at level 0 that the drive-out removes."""
    A, b, c, _ = lpcases.degenerate_eq_lp(seed, m=40, k=70, zero_rows=20)
    lo = np.zeros(70)
    hi = np.where(np.random.default_rng(seed + 99).random(70) < 0.5, 2.0, INF)
    return A, b, c, lo, hi, False


# (m, k, zero_rows, seed, draw) -> iters: found by a search on the reference over degenerate_eq_lp with random boxes (no
# case with both a drive-out pivot and a flip turned up at 40 x 70 in 400 seeds x 6 draws; these small ones did)
DRIVEOUT_FLIP = {(8, 16, 4, 223, 3): [11, 1, 1, 1], (8, 16, 4, 677, 0): [11, 1, 4, 1],
                 (16, 30, 8, 1979, 4): [32, 2, 2, 1], (16, 30, 8, 2197, 5): [30, 1, 4, 1]}


@functools.lru_cache(maxsize=None)
def driveout_with_flip(m, k, zero_rows, seed, draw):
    """lpcases.degenerate_eq_lp with the (draw+1)-th random boxes of default_rng(seed + 12345): negative lo on some
    columns, finite hi on others.  Phase I takes a flip and ends with an artificial basic at level 0, so the drive-out
    starts from a tableau with complemented columns."""
    A, b, c, _ = lpcases.degenerate_eq_lp(seed, m=m, k=k, zero_rows=zero_rows)
    rng = np.random.default_rng(seed + 12345)
    for _ in range(draw + 1):
        lo = np.where(rng.random(k) < 0.4, -rng.uniform(0.1, 1.0, k).round(2), 0.0)
        hi = np.where(rng.random(k) < 0.6, rng.uniform(0.3, 2.0, k).round(2), INF)
    return A, b, c, lo, hi, False


@functools.lru_cache(maxsize=None)
def identity_anchor(which):
    """lo = 0, hi = inf: (A, b, c, maximize, n_orig)."""
    if which == "gen":
        A, b, c, _, _, mx = boxed(160, 320, "mixed", 1)
        return A, b, c, mx, 160
    A, b, c, k = lpcases.min_lp(1, 40, 30, equalities=1, negative_rows=2, zero_rhs=1)
    return A, b, c, False, k


_ref_cache = {}


def ref(key, A, b, c, lo, hi, maximize, n_orig=None, eps=1e-9, max_iter=10000):
    """R.bounded(...), computed once per key."""
    if key not in _ref_cache:
        _ref_cache[key] = R.bounded(A, b, c, lo, hi, maximize, n_orig, eps, max_iter)
    return _ref_cache[key]
