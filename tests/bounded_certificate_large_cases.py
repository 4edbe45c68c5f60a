"""The inputs that tests/test_bounded_certificate_large_cpu.py and tests/test_gpu_bounded_certificate_large.py share, and
their reference certificates (tests/ref/bounded_certificate_ref.c; the solves by tests/ref/bounded_ref.c and
tests/ref/bounded_resolve_ref.c), computed once per process and never changed.  Test infrastructure only.

Every case is a dict(A, b, c, lo, hi, maximize, basis, at_upper, run) as in tests/bounded_certcases.py; the synthetic
families add `expect`, what their construction promises.
- cold, rich: bounded_certcases.cold and rich_unbounded at shapes beyond lp_basis_bounded_certificate_fits.
- contra: boxed_lp("mixed") with its last row replaced by row 0 and b[-1] = b[0] + 1: two rows that contradict each
  other, so phase I ends, after hundreds of pivots and flips, on a genuinely mixed basis with one artificial left.
- unreach: the "mixed" LP solved, then one basic column's lower bound raised beyond the largest value the column can
  take in the LP ("raise"), or its upper bound lowered beneath the smallest ("lower"): the bounded dual simplex runs
  until a position, usually another column's by then, cannot be brought back inside its bounds.
- tie_dual, tie_ray: synthetic bases of small dyadic data whose arithmetic is exact (the pattern of
  bounded_sens_large_cases.tie), built so that the winner is neither the first nor the last candidate and its rivals
  fail in different 256-column chunks or at the last positions.
"""
import functools

import numpy as np

from tests import bounded_certcases as BC
from tests import bounded_certificate_ref as CR
from tests import bounded_ref as B
from tests import bounded_resolve_ref as BR

OPTIMAL, UNBOUNDED, SINGULAR, INFEASIBLE, BAD_ARG = 0, 1, 3, 4, 5
NONE, FARKAS, RAY = CR.NONE, CR.FARKAS, CR.RAY

# 67 x 201 fits lp_basis_bounded_certificate_fits, the other shapes do not
COLD = [(kind, m, n, seed) for kind in ("infeasible", "unbounded") for (m, n, seed) in
        ((160, 320, 1), (160, 320, 2), (200, 500, 1))] + [("crossed", 160, 320, 1)]
RICH = [(67, 201, 1), (160, 320, 1), (200, 500, 1)]
CONTRA = [(67, 201, 1), (160, 320, 1), (160, 320, 2), (200, 500, 1)]
# (m, n, seed, move, side): the bound that moves ("raise" the lower bound, "lower" the upper bound) and the side on which
# the winning position, another column's after the dual pivots, ends up violated
UNREACH = [(67, 201, 2, "raise", "above"), (160, 320, 1, "raise", "above"), (160, 320, 2, "raise", "below"),
           (200, 500, 1, "raise", "below"), (67, 201, 2, "lower", "below")]
# (seed, m, n): seed 1 at 150 x 600 and seed 4 at 257 x 1030 have t3 above its upper bound, seed 2 below its lower bound
TIE_DUAL = [(1, 150, 600), (2, 257, 1030), (4, 257, 1030)]
# (seed, m, n, maximize)
TIE_RAY = [(1, 150, 600, False), (2, 150, 600, True), (1, 257, 1030, True), (3, 257, 1030, False)]
# the magnitude of the alpha entries that spoil rows t1 and t2 of tie_dual.  The violation is 1 (value -1.0), and at
# eps = 1 a position 1 outside its bound is no longer violated, so an integer magnitude cannot be reached by eps while
# the case stays a dual-simplex case: 0.5 is exact as well and lies below the violation.
SPOIL = 0.5


def _frozen(cs):
    for a in cs.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return cs


@functools.lru_cache(maxsize=None)
def cold(kind, m, n, seed):
    return _frozen(BC.cold(seed, m, n, kind))


@functools.lru_cache(maxsize=None)
def rich(m, n, seed):
    return _frozen(BC.rich_unbounded(seed, m, n))


@functools.lru_cache(maxsize=None)
def contra(m, n, seed):
    A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n, kind="mixed")
    A[-1] = A[0]
    b[-1] = b[0] + 1.0
    return _frozen(BC._case(A, b, c, lo, hi, mx, B.bounded(A, b, c, lo, hi, mx)))


@functools.lru_cache(maxsize=None)
def unreach(m, n, seed, move, side=None):
    """The first basic column, in position order, whose bound moved out of the column's reach makes the bounded dual
    simplex (bounded_resolve_ref.resolve from the optimal basis and flags) end INFEASIBLE.  The column's reach is found
    by the reference too: the re-solve of the same LP under the cost e_j from the optimal basis.  `side` is what the
    case is listed to show (tests/test_bounded_certificate_large_cpu.py asserts it); it is not used here."""
    A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n, kind="mixed")
    r = B.bounded(A, b, c, lo, hi, mx)
    assert r["status"] == OPTIMAL
    for t in range(m):
        j = int(r["basis"][t])
        if j >= n:
            continue
        e = np.zeros(n)
        e[j] = 1.0
        far = BR.resolve(A, b, e, lo, hi, r["basis"], r["at_upper"], move == "raise")
        if far["status"] != OPTIMAL:
            continue   # the column has no end on this side
        lo2, hi2 = lo.copy(), hi.copy()
        if move == "raise":
            lo2[j] = far["obj"] + 1.0
            hi2[j] = max(hi2[j], lo2[j] + 1.0)
        else:
            hi2[j] = far["obj"] - 1.0
            lo2[j] = min(lo2[j], hi2[j] - 1.0)
        g = BR.resolve(A, b, c, lo2, hi2, r["basis"], r["at_upper"], mx)
        if g["status"] == INFEASIBLE:
            return _frozen(dict(BC._case(A, b, c, lo2, hi2, mx, g), column=j, dual_pivots=g["iters"][0]))
    raise AssertionError("no basic column of this LP gives an infeasible re-solve")


def _tie_base(seed, m, n):
    """B a column-permuted unit lower bidiagonal matrix on m of the n columns, alpha_N small integers, bounds and flags;
    the caller shapes alpha_N, xB and c, then _tie_finish builds A and b."""
    rng = np.random.default_rng(seed)
    Bm = np.eye(m) + np.diag(rng.choice([-1.0, 1.0], m - 1), -1)
    Bm = Bm[:, rng.permutation(m)]
    cols = np.sort(rng.permutation(n)[:m])
    basis = cols[rng.permutation(m)].astype(np.int32)
    nonbasic = np.setdiff1d(np.arange(n), basis)
    alpha = rng.integers(-2, 3, (m, n - m)).astype(float)
    lo = rng.integers(-2, 1, n).astype(float)
    hi = np.where(rng.random(n) < 0.6, lo + rng.integers(2, 5, n), np.inf)
    up = ((rng.random(n) < 0.5) & np.isfinite(hi)).astype(np.int32)
    xB = np.minimum(lo[basis] + rng.integers(0, 3, m), hi[basis])
    return rng, Bm, basis, nonbasic, alpha, lo, hi, up, xB


def _tie_finish(Bm, basis, nonbasic, alpha, lo, hi, up, xB, c, maximize, expect):
    m, n = len(basis), len(lo)
    A = np.zeros((m, n))
    A[:, basis] = Bm
    A[:, nonbasic] = Bm @ alpha
    v = np.where(up == 1, hi, lo)
    v[basis] = 0.0
    b = Bm @ xB + A @ v
    return _frozen(dict(A=A, b=b, c=c, lo=lo, hi=hi, maximize=maximize, basis=basis, at_upper=up, run=INFEASIBLE
                        if expect["kind"] == FARKAS else UNBOUNDED, expect=expect, nonbasic=nonbasic, alpha=alpha))


@functools.lru_cache(maxsize=None)
def tie_dual(seed, m, n):
    """Four violated positions t1 = 5 < t2 = 70 < t3 = m-20 < t4 = m-3, each 1 outside its bound (t3 above when its
    upper bound is finite, the others below).  Their alpha rows carry the passing sign per column code; row t1 is
    spoiled (by SPOIL) in the last non-basic column only, row t2 in the first only.  Expected: FARKAS, index t3,
    value -1.0."""
    rng, Bm, basis, nonbasic, alpha, lo, hi, up, xB = _tie_base(seed, m, n)
    t1, t2, t3, t4 = 5, 70, m - 20, m - 3
    flagged = up[nonbasic] == 1
    sides = {}
    for t in (t1, t2, t3, t4):
        above = t == t3 and np.isfinite(hi[basis[t]])
        sides[t] = "above" if above else "below"
        xB[t] = hi[basis[t]] + 1.0 if above else lo[basis[t]] - 1.0
        mag = np.abs(alpha[t])
        alpha[t] = np.where(flagged != above, -mag, mag)   # below: >= 0 at lo, <= 0 at hi; above: the opposite
    alpha[t1, -1] = SPOIL if flagged[-1] else -SPOIL
    alpha[t2, 0] = SPOIL if flagged[0] else -SPOIL
    c = rng.integers(-3, 4, n).astype(float)
    expect = dict(kind=FARKAS, index=t3, value=-1.0, side=sides[t3], t=(t1, t2, t3, t4),
                  spoiled={t1: int(nonbasic[-1]), t2: int(nonbasic[0])})
    return _tie_finish(Bm, basis, nonbasic, alpha, lo, hi, up, xB, c, False, expect)


@functools.lru_cache(maxsize=None)
def tie_ray(seed, m, n, maximize):
    """No position is violated and no column qualifies, except four unflagged columns j1 < j2 < j3 < j4 without an
    upper bound whose d_j = s (k+1) improves (s = +1 to maximize, -1 to minimize) and whose alpha columns are
    non-positive integers, non-zero only where H_t = +inf.  j1 is spoiled by a +1 in one of the last two positions, j2
    by a -1 at the last position with a finite H_t.  Expected: RAY, index j3, value 3 s; j4 qualifies too."""
    rng, Bm, basis, nonbasic, alpha, lo, hi, up, xB = _tie_base(seed, m, n)
    s = 1.0 if maximize else -1.0
    c = rng.integers(-3, 4, n).astype(float)
    cB = c[basis]
    free = np.isinf(hi[basis])   # by position: H_t = +inf
    picks = [int(len(nonbasic) * q) for q in (0.1, 0.35, 0.6, 0.9)]
    for k, q in enumerate(picks):
        j = nonbasic[q]
        hi[j], up[j] = np.inf, 0
        alpha[:, q] = np.where(free, -rng.integers(0, 3, m), 0).astype(float)
    last_finite = int(np.flatnonzero(~free)[-1])
    alpha[m - 1 - int(rng.integers(0, 2)), picks[0]] = 1.0
    alpha[last_finite, picks[1]] = -1.0
    c[nonbasic] = cB @ alpha - s * rng.integers(0, 3, n - m)
    for k, q in enumerate(picks):
        c[nonbasic[q]] = cB @ alpha[:, q] + s * (k + 1)
    js = tuple(int(nonbasic[q]) for q in picks)
    expect = dict(kind=RAY, index=js[2], value=3.0 * s, j=js)
    return _tie_finish(Bm, basis, nonbasic, alpha, lo, hi, up, xB, c, bool(maximize), expect)


def at(cs):
    """The certificate entries' leading arguments of a case."""
    return cs["A"], cs["b"], cs["c"], cs["lo"], cs["hi"], cs["basis"], cs["at_upper"]


def all_cases():
    """(id, builder) of every case the GPU test runs."""
    out = [("cold-%s-%dx%d-%d" % k, functools.partial(cold, *k)) for k in COLD]
    out += [("rich-%dx%d-%d" % k, functools.partial(rich, *k)) for k in RICH]
    out += [("contra-%dx%d-%d" % k, functools.partial(contra, *k)) for k in CONTRA]
    out += [("unreach-%dx%d-%d-%s-%s" % k, functools.partial(unreach, *k)) for k in UNREACH]
    out += [("tie_dual-%d-%dx%d" % k, functools.partial(tie_dual, *k)) for k in TIE_DUAL]
    out += [("tie_ray-%d-%dx%d-%s" % k, functools.partial(tie_ray, *k)) for k in TIE_RAY]
    return out


_cache = {}


def ref(key, cs, eps=1e-9, maximize=None):
    """The reference certificate of a case, computed once per (key, eps, maximize)."""
    mx = cs["maximize"] if maximize is None else bool(maximize)
    k = (key, eps, mx)
    if k not in _cache:
        _cache[k] = CR.certificate(*at(cs), mx, eps)
    return _cache[k]
