"""The inputs that tests/test_bounded_parametric_large_cpu.py and tests/test_gpu_bounded_parametric_large.py share, and
their reference results (tests/ref/bounded_parametric_ref.c through tests/bounded_parametric_ref.py), computed once per
key and never changed.  A case is (A, b, c, lo, hi, basis, at_upper, direction, maximize).  Test infrastructure only."""
import functools

import numpy as np

from tests import bounded_parametric_ref as P

INF = np.inf
OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
PATHS = P.PATHS

BEYOND_BREAKS = 400
# (path, m, n, seed, maximize, kind): beyond lp_basis_bounded_parametric_fits, except 67 x 201, which fits and is here
# for its odd row length and for the comparison with the LDS entry
BEYOND = [(path, 160, 320, s, mx, "mixed") for path in PATHS for s in (1, 2, 3, 4) for mx in (True, False)]
BEYOND += [(path, 200, 500, 1, mx, "mixed") for path in PATHS for mx in (True, False)]
BEYOND += [(path, 67, 201, s, mx, "mixed") for path in PATHS for s in (1, 2) for mx in (True, False)]
LIMIT = ("rhs", 200, 500, 4, False, "mixed")    # the reference walks into max_breaks = 400 here
RAY = ("cost", 160, 320, 1, True, "ray")        # ends LP_UNBOUNDED
BEYOND += [LIMIT, RAY]

TALL_SHAPE = (1100, 2300)
TALL_BREAKS = 60
TALL_SEED = 7
TIE_ROWS = (3, 1050)        # RHS: b = 0.125, d = -8.0 in both: tau = 1/64 in both
TIE_COLS = (5, 1100)        # cost: equal columns of A, equal hi, c = 0.25, g = -16.0: tau = 1/64 in both
TALL = [(path, reverse) for path in PATHS for reverse in (False, True)]


def _freeze(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(arrays)


def key_id(key):
    return "-".join(str(k) for k in key)


@functools.lru_cache(maxsize=None)
def beyond(path, m, n, seed, maximize, kind="mixed"):
    case = P.boxed_case(path, seed, m, n, maximize, kind)
    assert case is not None, "the cold solve is not optimal"
    return _freeze(list(case))


@functools.lru_cache(maxsize=None)
def tall(path, reverse):
    """More basis positions and more columns than the selectors have threads: a minimisation from the slack basis (in
    order: the crash is skipped; reversed: the crash and the row permutation run), optimal at t = 0 because every
    structural cost is positive and b lies inside the slacks' boxes.  The first breakpoint is an exact tie of two tau
    candidates, two positions (RHS path) or two columns (cost path), across the 1024 stride of the gather, which runs
    on all 1024 threads.  The entering chain and the ratio test behind it run on 960 threads and are replayed in tiles
    of 1024: their seams are pinned by tests/bounded_parametric_seam_cases.py."""
    m, n = TALL_SHAPE
    rng = np.random.default_rng(TALL_SEED)
    k = n - m
    A = np.hstack([rng.uniform(-1, 1, (m, k)).round(2), np.eye(m)])
    c = np.concatenate([rng.uniform(.1, 1, k).round(2), np.zeros(m)])
    b = rng.uniform(.05, .45, m).round(2)
    lo, hi = np.zeros(n), np.full(n, INF)
    hi[k:] = np.where(rng.random(m) < .5, .5, INF)
    hi[:k] = np.where(rng.random(k) < .5, .02, INF)
    basis = np.arange(k, n, dtype=np.int32)
    if reverse:
        basis = basis[::-1].copy()
    if path == "rhs":
        direction = rng.uniform(-1.0, 1.0, m) * np.abs(b)
        for t in TIE_ROWS:
            b[t], direction[t] = 0.125, -8.0
    else:
        direction = rng.uniform(-1.0, 1.0, n) * (np.abs(c) + 0.25)
        direction[k:] = 0.0   # (both cost rows are zero on the slack basis)
        j0, j1 = TIE_COLS
        A[:, j1] = A[:, j0]
        hi[j1] = hi[j0]
        for j in TIE_COLS:
            c[j], direction[j] = 0.25, -16.0
    return _freeze([A, b, c, lo, hi, basis, np.zeros(n, np.int32), direction, False])


def all_cases():
    """(id, path, make, max_breaks) of every case the GPU test compares with the reference."""
    out = [(key_id(k), k[0], functools.partial(beyond, *k), BEYOND_BREAKS) for k in BEYOND]
    out += [("tall-%s-%s" % (path, "reversed" if rev else "in-order"), path, functools.partial(tall, path, rev),
             TALL_BREAKS) for path, rev in TALL]
    return out


_ref_cache = {}


def ref(key, path, case, eps=1e-9, max_breaks=BEYOND_BREAKS, t_max=INF):
    """P.parametric(path, *case, ...), computed once per key."""
    full = (key, path, eps, max_breaks, t_max)
    if full not in _ref_cache:
        _ref_cache[full] = P.parametric(path, *case[:8], t_max=t_max, maximize=case[8], eps=eps, max_breaks=max_breaks)
    return _ref_cache[full]
