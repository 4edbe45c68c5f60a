"""The inputs that tests/test_bounded_sens_large_cpu.py and tests/test_gpu_bounded_sens_large.py share, and their
reference results (tests/ref/bounded_ref.c for the solves, tests/ref/bounded_sens_ref.c for the analyses), computed once
per process and never changed.  Test infrastructure only."""
import functools

import numpy as np

from tests import bounded_large_cases as Q
from tests import bounded_sens_ref as S

OPTIMAL = 0

# (m, n, kind, seed) of bounded_large_cases.boxed: 67 x 201 fits lp_basis_bounded_fits, the other shapes do not
SOLVED = [(67, 201, "mixed", 1), (67, 201, "mixed", 2), (160, 320, "mixed", 1), (160, 320, "mixed", 2),
          (160, 320, "box", 1), (160, 320, "box", 2), (200, 500, "mixed", 1)]

# (seed, m, n) of tie(): 257 x 1030 crosses every block boundary of the HBM kernels (64 rows, 64 x 64 tiles, 256-column
# chunks) with a remainder.  (Seed 2 at 150 x 600 has no basic column whose winning cost ratio is attained in two
# 256-column chunks, which tests/test_bounded_sens_large_cpu.py asks of every case; seed 5 has.)
TIES = [(1, 150, 600), (5, 150, 600), (3, 257, 1030)]


@functools.lru_cache(maxsize=None)
def solved_ref(m, n, kind, seed):
    """The reference solve (tests/ref/bounded_ref.c) of a SOLVED case."""
    A, b, c, lo, hi, mx = Q.boxed(m, n, kind, seed)
    return Q.ref(("sens-large", m, n, kind, seed), A, b, c, lo, hi, mx)


@functools.lru_cache(maxsize=None)
def tie(seed, m, n):
    """(A, b, c, lo, hi, basis, at_upper): a synthetic basis of integer data whose arithmetic is exact.  B is a
    column-permuted unit lower bidiagonal matrix, so B^-1 has entries 0 and +-1 and xB lies 0 to 2 above its lower
    bound: most rows' lower RHS end is attained by several positions at once."""
    rng = np.random.default_rng(seed)
    Bm = np.eye(m) + np.diag(rng.choice([-1.0, 1.0], m - 1), -1)
    Bm = Bm[:, rng.permutation(m)]
    cols = np.sort(rng.permutation(n)[:m])
    basis = cols[rng.permutation(m)].astype(np.int32)
    A = rng.integers(-2, 3, (m, n)).astype(float)
    A[:, basis] = Bm
    c = rng.integers(-3, 4, n).astype(float)
    lo = rng.integers(-2, 1, n).astype(float)
    hi = np.where(rng.random(n) < 0.6, lo + rng.integers(2, 5, n), np.inf)
    up = ((rng.random(n) < 0.5) & np.isfinite(hi)).astype(np.int32)
    v = np.where(up == 1, hi, lo)
    v[basis] = 0
    b = A[:, basis] @ (lo[basis] + rng.integers(0, 3, m)) + A @ v
    case = (A, b, c, lo, hi, basis, up)
    for a in case:
        a.setflags(write=False)
    return case


_cache = {}


def duals(key, *at):
    """S.duals(*at), computed once per key."""
    if ("d", key) not in _cache:
        _cache[("d", key)] = S.duals(*at)
    return _cache[("d", key)]


def ranging(key, *at, maximize=False, eps=1e-9):
    """S.ranging(*at, maximize, eps), computed once per (key, maximize, eps)."""
    k = ("r", key, bool(maximize), eps)
    if k not in _cache:
        _cache[k] = S.ranging(*at, maximize, eps)
    return _cache[k]
