"""Inputs that put the scans of lp_basis_bounded_parametric_large and lp_basis_bounded_parametric_cost_large at
near-ties across the places where their work is cut.  A selector gathers its tau candidates on all 1024 threads (entry j
sits in wave (j % GATHER) / 64, and wave 15 leaves after storing its candidate), runs the entering chain over row r
(RHS path) or the bounded ratio test over column e (cost path) on SCAN = 960 threads (thread t holds entries t, t + 960,
t + 1920; the near check strides by 960) with a replay that walks tiles of TILE = 1024, stages lcol and prow and flips a
bound with a stride of 960, and adds the held non-basic columns to the objective chain CHUNK = 256 columns at a time.

Every case is a minimisation with lo = 0 from the slack basis, at 1100 x 2300 (rows and columns across 960 and 1024),
24 x 4300 (columns across 1920 and 2048), 2060 x 2080 (rows across 1920 and 2048) and, where the crash runs,
1100 x 1140.  TALL has 1100 rows, so the row pairs of the cost path stop at 1099: (1030, 1094) is its pair in the same
lane of neighbouring waves, and its carry and late pairs sit at 1090 and 1091.  In order the crash is skipped, the
tableau at t = 0 is A itself and the reduced costs are c, so the first breakpoint (t = 1/64) is written down exactly:
small dyadic values at the pinned entries make the pinned quotients exact.  Later breakpoints come from seeded random
data.  What every case promises (the seam relation of its pinned indices, its first breakpoint at eps = 0 and 1e-12) is
kept beside it and asserted on the reference alone in tests/test_bounded_parametric_seams_cpu.py;
tests/test_gpu_bounded_parametric_seams.py compares the kernels with the reference over GRID.
A case is (A, b, c, lo, hi, basis, at_upper, direction, maximize).  Test infrastructure only."""
import collections
import functools

import numpy as np

from tests import bounded_parametric_large_cases as L

INF = np.inf
SCAN, TILE, GATHER, CHUNK = 960, 1024, 1024, 256
# SLIM: TALL's rows with 40 structurals, for the cases whose crash runs (the reference's crash costs m pivots over
# the whole tableau, more than a second per call at TALL)
SHAPES = dict(TALL=(1100, 2300), WIDE=(24, 4300), DEEP=(2060, 2080), SLIM=(1100, 1140))
EPS = (0.0, 1e-12, 1e-2)
BREAKS = (0, 1, 8)
GRID = [(eps, mb) for eps in EPS for mb in BREAKS]
SEED = 11
TAU = 1.0 / 64

ONE_LO = np.nextafter(1.0, 0.0)
Q, Q_LO, Q_HI = 0.25, np.nextafter(0.25, 0.0), np.nextafter(0.25, 1.0)
HALF_UP = 0.5 + 2.0 ** -41          # within 1e-12 of 0.5, and exact
FLAG_HI = 2.0 ** -6                 # the upper bound of the one flagged column a pinned row keeps: b' stays exact

# name, path, shape, make() -> the case, space: what the pinned indices are ("col" / "pos": the entering chain's columns
# or the ratio test's positions; "tau": positions (RHS) or columns (cost) of the gather), pair, rel: names of RELATIONS
# that hold for pair, first: eps -> (enter[0], leave[0], side[0]) at max_breaks >= 1, near: the two eps give different
# answers, flip: eps -> the first breakpoint is a bound flip (cost path), flagged: the structurals start flagged
Case = collections.namedtuple("Case", "name path shape make space pair rel first near flip flagged reverse")


def wave_of(j):
    return (j % GATHER) // 64


RELATIONS = {
    "same_thread": lambda p, q: p != q and p % SCAN == q % SCAN,
    "straddle_scan": lambda p, q: p // SCAN != q // SCAN,
    "straddle_scan2": lambda p, q: p < 2 * SCAN <= q,
    "straddle_tile": lambda p, q: p // TILE != q // TILE,
    "straddle_tile2": lambda p, q: p < 2 * TILE <= q,
    "same_scan_step": lambda p, q: p // SCAN == q // SCAN,
    "same_tile": lambda p, q: p // TILE == q // TILE,
    "adjacent": lambda p, q: q == p + 1,
    "beyond_scan": lambda p, q: SCAN <= p < q,
    "beyond_tile": lambda p, q: TILE <= p < q,
    "beyond_scan2": lambda p, q: 2 * SCAN <= p < q,
    "beyond_tile2": lambda p, q: 2 * TILE <= p < q,
    "third_entry": lambda p, q: q // SCAN == 2,
    "third_tile": lambda p, q: q // TILE == 2,
    # the same lane of neighbouring scan waves, the smaller index in the earlier wave
    "next_wave_same_lane": lambda p, q: (q % SCAN) - (p % SCAN) == 64 and p // SCAN == q // SCAN,
    "first_in_tile0": lambda p, q: p < TILE,
    "winner_wave15": lambda p, q: wave_of(p) == 15,
    "loser_wave15": lambda p, q: wave_of(q) == 15,
    "loser_wave0": lambda p, q: wave_of(q) == 0,
    "winner_not_wave15": lambda p, q: wave_of(p) != 15,
    "second_gather_step": lambda p, q: p < GATHER <= q,
    "lone_wave15": lambda p, q: q is None and wave_of(p) == 15 and p >= SCAN,
}


@functools.lru_cache(maxsize=None)
def _structurals(shape):
    m, n = SHAPES[shape]
    S = np.random.default_rng(SEED).uniform(-1, 1, (m, n - m)).round(2)
    S.setflags(write=False)
    return S


def _flags(rng, k, unflagged):
    """About 40 % of the structurals, with neighbours across every 256-column chunk edge that matters and the last."""
    f = rng.random(k) < 0.4
    for j in (CHUNK - 1, CHUNK, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, k - 1):
        if j < k:
            f[j] = True
    f[list(unflagged)] = False
    return f


def _finish(A, b, c, lo, hi, up, direction, reverse):
    m, n = A.shape
    basis = np.arange(n - m, n, dtype=np.int32)
    if reverse:
        basis = basis[::-1].copy()
    return L._freeze([A, b, c, lo, hi, basis, up, direction, False])


def rhs_case(shape, rows, flagged=False, reverse=False, others="none", dup=None):
    """rows: (position, above, slack_up, {column: (a, cost)}).  The row at that basis position blocks at t = 1/64: below
    (beta = 0.125, delta = -8), or above (hi = 1, beta = 0.875, delta = 8; the row is read complemented); slack_up:
    its slack starts flagged at hi = 1, so the tableau holds the row negated and side = 1 ^ above.  What the entering
    chain READS in that row is >= 0 (ineligible) everywhere except at the given columns, which read a and cost `cost`.
    others: the other rows are no tau candidates ("none": delta >= 0 without an upper bound, or delta = 0 with one) or
    clear losers on half of them ("losers": tau >= 2.5).  dup: (j0, j1), column j1 becomes a copy of column j0."""
    m, n = SHAPES[shape]
    k = n - m
    rng = np.random.default_rng(SEED + 1)
    A = np.hstack([_structurals(shape), np.eye(m)])
    c = np.concatenate([rng.uniform(0.1, 1, k).round(2), np.zeros(m)])
    b = rng.uniform(0.05, 0.45, m).round(2)
    lo, hi, up = np.zeros(n), np.full(n, INF), np.zeros(n, np.int32)
    d = rng.uniform(0, 1, m) * b
    boxed = rng.random(m) < 0.3
    hi[k:][boxed] = 0.5
    d[boxed] = 0.0
    lose = ~boxed & (rng.random(m) < 0.5)
    scale = rng.uniform(0.1, 0.4, m)
    if others == "losers":
        d[lose] = -b[lose] * scale[lose]
    hi[:k] = np.where(rng.random(k) < 0.5, 0.02, INF)
    pinned = sorted({j for r in rows for j in r[3]} | set(dup or ()))
    f = _flags(rng, k, pinned) if flagged else np.zeros(k, bool)
    hi_f = rng.uniform(0.01, 0.02, k).round(3)
    jf = int(np.flatnonzero(f)[3]) if flagged else -1
    if flagged:
        hi[:k][f] = hi_f[f]
        c[:k][f] *= -1.0
        up[:k][f] = 1
        hi[jf], c[jf] = FLAG_HI, -3.0      # eligible in the pinned rows, a clear loser (quotient 3)
    for pos, above, slack_up, entries in rows:
        i = m - 1 - pos if reverse else pos
        read = np.abs(A[i, :k])
        read[f] = 0.0
        if flagged:
            read[jf] = -1.0
        for j, (a, cost) in entries.items():
            read[j], c[j], hi[j] = a, cost, INF
        sign = (-1.0 if above else 1.0) * (-1.0 if slack_up else 1.0)
        A[i, :k] = read * np.where(f, -1.0, 1.0) * sign + 0.0
        down = above == slack_up            # the slack itself heads for its lower bound
        b[i], d[i] = (0.125, -8.0) if down else (0.875, 8.0)
        hi[k + i] = 1.0 if (above or slack_up) else INF
        up[k + i] = 1 if slack_up else 0
    if dup:
        j0, j1 = dup
        A[:, j1], c[j1], hi[j1] = A[:, j0], c[j0], hi[j0]
    if flagged:
        b = b + A[:, :k][:, f] @ hi[:k][f]
    return _finish(A, b, c, lo, hi, up, d, reverse)


def cost_case(shape, ents, rows, hi_e=INF, flagged=False, reverse=False, lone=False, nonzero=()):
    """ents: the entering column (c = 0.25, g = -16: tau = 1/64) and its exact copies; every other column is a clear
    loser (tau >= 2) or, with lone, no candidate.  rows: position -> (a, b, hi of its slack): the rows of the entering
    column that the ratio test may take; every other row holds a <= 0 on a slack without an upper bound, or 0 on one
    with hi = 0.5.  hi_e: the entering column's upper bound (the flip against the pivot).  nonzero: positions that get
    a = -0.5 (rows a bound flip must rewrite)."""
    m, n = SHAPES[shape]
    k = n - m
    rng = np.random.default_rng(SEED + 2)
    A = np.hstack([_structurals(shape), np.eye(m)])
    c = np.concatenate([rng.uniform(2, 3, k).round(2), np.zeros(m)])
    g = np.concatenate([rng.uniform(-1, 1, k).round(3), np.zeros(m)])
    b = rng.uniform(0.05, 0.45, m).round(2)
    lo, hi, up = np.zeros(n), np.full(n, INF), np.zeros(n, np.int32)
    boxed = rng.random(m) < 0.3
    hi[k:][boxed] = 0.5
    hi[:k] = np.where(rng.random(k) < 0.5, 0.02, INF)
    f = _flags(rng, k, ents) if flagged else np.zeros(k, bool)
    hi_f = rng.uniform(0.01, 0.02, k).round(3)
    if lone:
        g[:k] = np.abs(g[:k])
    if flagged:
        hi[:k][f] = hi_f[f]
        c[:k][f] *= -1.0
        up[:k][f] = 1
        if lone:
            g[:k][f] *= -1.0
    row = (lambda pos: m - 1 - pos) if reverse else (lambda pos: pos)
    e = ents[0]
    col = -np.abs(A[:, e])
    col[boxed] = 0.0
    for pos in nonzero:
        col[row(pos)], hi[k + row(pos)] = -0.5, INF
    for pos, (a, bv, sh) in rows.items():
        i = row(pos)
        col[i], b[i], hi[k + i] = a, bv, sh
        A[i, :k][f] = 0.0                   # b' stays exact in the pinned rows
    for j in ents:
        A[:, j], c[j], g[j], hi[j] = col + 0.0, 0.25, -16.0, hi_e
    if flagged:
        b = b + A[:, :k][:, f] @ hi[:k][f]
    return _finish(A, b, c, lo, hi, up, g, reverse)


# ---- the catalogue ---------------------------------------------------------------------------------------------------

CASES = collections.OrderedDict()


def _add(name, path, shape, make, space, pair, rel, first, near, flip=None, flagged=False, reverse=False):
    assert name not in CASES, name
    CASES[name] = Case(name, path, shape, make, space, pair, tuple(rel), first, near, flip, flagged, reverse)


def _var(shape, pos, reverse=False):
    """The slack that sits at a basis position."""
    m, n = SHAPES[shape]
    return n - m + (m - 1 - pos if reverse else pos)


def _rhs_pair(family, shape, r, pair, rel, above=False, slack_up=False, flagged=False, reverse=False):
    p, q = pair
    tag = "%s@%d,%d-%s%s%s%s%s" % (family, p, q, shape, "-above" if above else "", "-slackup" if slack_up else "",
                                   "-flagged" if flagged else "", "-reversed" if reverse else "")
    make = functools.partial(rhs_case, shape, ((r, above, slack_up, {p: (-1.0, 1.0), q: (-1.0, ONE_LO)}),),
                             flagged=flagged, reverse=reverse)
    leave, side = _var(shape, r, reverse), int(slack_up) ^ int(above)
    _add("rhs-" + tag, "rhs", shape, make, "col", pair, rel, {0.0: (q, leave, side), 1e-12: (p, leave, side)}, True,
         flagged=flagged, reverse=reverse)


def _rhs_catalogue():
    R, RA = 1050, 990                      # the blocking position, below and above (both past the scan's 960 threads)
    for above in (False, True):
        r = RA if above else R
        _rhs_pair("same_thread", "TALL", r, (40, 1000) if above else (3, 963), ("same_thread", "straddle_scan"), above)
        _rhs_pair("straddle_tile", "TALL", r, (1023, 1024), ("straddle_tile", "adjacent", "beyond_scan"), above)
        _rhs_pair("beyond", "TALL", r, (1030, 1031), ("beyond_tile", "adjacent", "same_tile"), above)
        _rhs_pair("beyond", "TALL", r, (1040, 1104), ("beyond_tile", "next_wave_same_lane"), above)
    _rhs_pair("straddle_scan", "TALL", R, (959, 960), ("straddle_scan", "adjacent", "same_tile"))
    _rhs_pair("between", "TALL", R, (970, 1010), ("beyond_scan", "same_tile", "first_in_tile0"))
    _rhs_pair("between_tiles", "TALL", RA, (1000, 1030), ("beyond_scan", "straddle_tile"), above=True)
    W = 20
    _rhs_pair("same_thread", "WIDE", W, (10, 1930), ("same_thread", "straddle_scan2", "third_entry"))
    _rhs_pair("straddle_scan", "WIDE", W, (1919, 1920), ("straddle_scan2", "adjacent", "third_entry"))
    _rhs_pair("between", "WIDE", W, (1930, 2050), ("beyond_scan2", "straddle_tile2", "third_tile"))
    _rhs_pair("straddle_tile", "WIDE", W, (2047, 2048), ("straddle_tile2", "adjacent", "third_tile"))
    _rhs_pair("beyond", "WIDE", W, (2100, 2101), ("beyond_tile2", "beyond_scan2", "adjacent"))
    # carry: the replay must carry `best` from tile 0 into tile 1; late_pair: its mirror
    lv = _var("TALL", R)
    _add("rhs-carry@100,200,1100-TALL", "rhs", "TALL",
         functools.partial(rhs_case, "TALL", ((R, False, False, {100: (-1.0, 1.0), 200: (-1.0, HALF_UP),
                                                                  1100: (-1.0, 0.5)}),)),
         "col", (200, 1100), ("straddle_tile", "straddle_scan"), {0.0: (1100, lv, 0), 1e-12: (200, lv, 0)}, True)
    _add("rhs-late_pair@100,1100,1101-TALL", "rhs", "TALL",
         functools.partial(rhs_case, "TALL", ((R, False, False, {100: (-1.0, 2.0), 1100: (-1.0, 1.0),
                                                                  1101: (-1.0, ONE_LO)}),)),
         "col", (1100, 1101), ("beyond_tile", "adjacent"), {0.0: (1101, lv, 0), 1e-12: (1100, lv, 0)}, True)
    # exact copies, cost included: the first index wins at every eps
    _add("rhs-dup@40,1000-TALL", "rhs", "TALL",
         functools.partial(rhs_case, "TALL", ((R, False, False, {40: (-1.0, 1.0)}),), dup=(40, 1000)),
         "col", (40, 1000), ("same_thread",), {0.0: (40, lv, 0), 1e-12: (40, lv, 0)}, False)
    _add("rhs-dup@1000,1960-WIDE", "rhs", "WIDE",
         functools.partial(rhs_case, "WIDE", ((W, False, False, {1000: (-1.0, 1.0)}),), dup=(1000, 1960)),
         "col", (1000, 1960), ("same_thread", "straddle_scan2", "straddle_tile"),
         {0.0: (1000, _var("WIDE", W), 0), 1e-12: (1000, _var("WIDE", W), 0)}, False)
    # the blocking row has no entry to enter with: the path ends LP_INFEASIBLE at the first breakpoint
    _add("rhs-no_entering@1050-TALL", "rhs", "TALL", functools.partial(rhs_case, "TALL", ((R, False, False, {}),)),
         "tau", (R, None), (), {0.0: (-1, lv, 0), 1e-12: (-1, lv, 0)}, False)
    # flagged starts: the chain wave's column part adds something at t = 0
    _rhs_pair("beyond", "TALL", R, (1030, 1031), ("beyond_tile", "adjacent"), flagged=True)
    _rhs_pair("beyond", "WIDE", W, (2100, 2101), ("beyond_tile2", "adjacent"), flagged=True)
    _rhs_pair("beyond", "TALL", RA, (1040, 1104), ("beyond_tile", "next_wave_same_lane"), above=True, slack_up=True,
              flagged=True)
    # reversed (the crash runs and the rows are permuted): columns stay where they are, so on this path the reversal
    # moves the tau candidates alone (the tie below)

    # the gather: exact ties of two positions (tau = 1/64 in both); each brings its own entering column
    def tie(shape, pair, rel, above=(False, False), reverse=False, name="tau_tie"):
        p, q = pair
        rows = ((p, above[0], False, {3: (-1.0, 1.0)}), (q, above[1], False, {5: (-1.0, 1.0)}))
        tag = "rhs-%s@%d,%d-%s%s" % (name, p, q, shape, "-reversed" if reverse else "")
        first = (3, _var(shape, p, reverse), int(above[0]))
        _add(tag, "rhs", shape, functools.partial(rhs_case, shape, rows, others="losers", reverse=reverse), "tau",
             pair, rel, {0.0: first, 1e-12: first}, False, reverse=reverse)
    for shape in ("TALL", "DEEP"):
        tie(shape, (1000, 1030), ("winner_wave15", "loser_wave0", "second_gather_step"))
        tie(shape, (70, 1030), ("winner_not_wave15", "loser_wave0", "second_gather_step"))
    tie("DEEP", (990, 2014), ("winner_wave15", "loser_wave15"))
    tie("TALL", (1000, 1030), ("winner_wave15", "loser_wave0"), above=(False, True), name="tau_below_above")
    tie("TALL", (1000, 1030), ("winner_wave15", "loser_wave0"), above=(True, False), name="tau_above_below")
    tie("SLIM", (1000, 1030), ("winner_wave15", "loser_wave0"), reverse=True)
    lone = _var("TALL", 1010)
    _add("rhs-tau_lone@1010-TALL", "rhs", "TALL",
         functools.partial(rhs_case, "TALL", ((1010, False, False, {3: (-1.0, 1.0)}),)), "tau", (1010, None),
         ("lone_wave15",), {0.0: (3, lone, 0), 1e-12: (3, lone, 0)}, False)


def _cost_pair(family, shape, pair, rel, kind="low_low", hi_e=INF, flagged=False, reverse=False, nonzero=(), e=7,
               first=None, near=True, flip=None):
    p, q = pair
    rows = {"low_low": {p: (1.0, Q, INF), q: (1.0, Q_LO, INF)},
            "low_up": {p: (1.0, Q, INF), q: (-1.0, Q_HI, 0.5)},
            "up_up": {p: (-1.0, Q, 0.5), q: (-1.0, Q_HI, 0.5)}}[kind]
    sides = {"low_low": (0, 0), "low_up": (0, 1), "up_up": (1, 1)}[kind]
    tag = "cost-%s@%d,%d-%s%s%s" % (family, p, q, shape, "-flagged" if flagged else "", "-reversed" if reverse else "")
    make = functools.partial(cost_case, shape, (e,), rows, hi_e=hi_e, flagged=flagged, reverse=reverse, nonzero=nonzero)
    if first is None:
        first = {0.0: (e, _var(shape, q, reverse), sides[1]), 1e-12: (e, _var(shape, p, reverse), sides[0])}
    _add(tag, "cost", shape, make, "pos", pair, rel, first, near, flip=flip, flagged=flagged, reverse=reverse)


def _cost_catalogue():
    _cost_pair("same_thread", "TALL", (30, 990), ("same_thread", "straddle_scan"))
    _cost_pair("straddle_scan", "TALL", (959, 960), ("straddle_scan", "adjacent", "same_tile"))
    _cost_pair("straddle_tile", "TALL", (1023, 1024), ("straddle_tile", "adjacent", "beyond_scan"))
    _cost_pair("between", "TALL", (970, 1010), ("beyond_scan", "same_tile", "first_in_tile0"))
    _cost_pair("between_tiles", "TALL", (1000, 1030), ("beyond_scan", "straddle_tile"))
    _cost_pair("beyond", "TALL", (1030, 1031), ("beyond_tile", "adjacent", "same_tile"))
    _cost_pair("beyond", "TALL", (1030, 1094), ("beyond_tile", "next_wave_same_lane"))
    _cost_pair("same_thread", "DEEP", (100, 2020), ("same_thread", "straddle_scan2", "straddle_tile", "third_entry"))
    _cost_pair("straddle_scan", "DEEP", (1919, 1920), ("straddle_scan2", "adjacent", "third_entry"))
    _cost_pair("straddle_tile", "DEEP", (2047, 2048), ("straddle_tile2", "adjacent", "third_tile"))
    _cost_pair("beyond", "DEEP", (2050, 2051), ("beyond_tile2", "beyond_scan2", "adjacent"))
    _cost_pair("low_up", "TALL", (1030, 1094), ("beyond_tile", "next_wave_same_lane"), kind="low_up")
    _cost_pair("up_up", "TALL", (1023, 1024), ("straddle_tile", "adjacent"), kind="up_up")
    # the flip against the pivot: U_e just below, at and just above the pair's ratios
    fp, m = (1030, 1093), SHAPES["TALL"][0]
    nz = (965, 1025, m - 1)
    e = 7
    flipped, lp, lq = (e, e, 1), (e, _var("TALL", fp[0]), 0), (e, _var("TALL", fp[1]), 0)
    _cost_pair("flip_below", "TALL", fp, ("beyond_tile",), hi_e=Q_LO, nonzero=nz, first={0.0: flipped, 1e-12: flipped},
               near=False, flip={0.0: True, 1e-12: True})
    _cost_pair("flip_equal", "TALL", fp, ("beyond_tile",), hi_e=Q, nonzero=nz, first={0.0: lq, 1e-12: flipped},
               flip={0.0: False, 1e-12: True})
    _cost_pair("flip_above", "TALL", fp, ("beyond_tile",), hi_e=Q_HI, nonzero=nz, first={0.0: lq, 1e-12: lp},
               flip={0.0: False, 1e-12: False})
    v = functools.partial(_var, "TALL")
    _add("cost-carry_rows@100,200,1090-TALL", "cost", "TALL",
         functools.partial(cost_case, "TALL", (e,), {100: (1.0, 1.0, INF), 200: (1.0, HALF_UP, INF),
                                                     1090: (1.0, 0.5, INF)}),
         "pos", (200, 1090), ("straddle_tile", "straddle_scan"), {0.0: (e, v(1090), 0), 1e-12: (e, v(200), 0)}, True)
    _add("cost-late_pair_rows@100,1090,1091-TALL", "cost", "TALL",
         functools.partial(cost_case, "TALL", (e,), {100: (1.0, 1.0, INF), 1090: (1.0, Q, INF),
                                                     1091: (1.0, Q_LO, INF)}),
         "pos", (1090, 1091), ("beyond_tile", "adjacent"), {0.0: (e, v(1091), 0), 1e-12: (e, v(1090), 0)}, True)
    _add("cost-dup_rows@40,1000-TALL", "cost", "TALL",
         functools.partial(cost_case, "TALL", (e,), {40: (1.0, Q, INF), 1000: (1.0, Q, INF)}),
         "pos", (40, 1000), ("same_thread",), {0.0: (e, v(40), 0), 1e-12: (e, v(40), 0)}, False)
    _cost_pair("beyond", "TALL", (1030, 1031), ("beyond_tile", "adjacent"), flagged=True)
    _cost_pair("between", "WIDE", (3, 17), ("same_tile",), flagged=True, e=2100)
    _cost_pair("same_thread", "SLIM", (30, 990), ("same_thread", "straddle_scan"), reverse=True)
    _cost_pair("beyond", "SLIM", (1030, 1031), ("beyond_tile", "adjacent"), reverse=True)
    fr = lambda pos: _var("SLIM", pos, True)   # noqa: E731
    _cost_pair("flip_equal", "SLIM", fp, ("beyond_tile",), hi_e=Q, nonzero=nz, reverse=True,
               first={0.0: (e, fr(fp[1]), 0), 1e-12: flipped}, flip={0.0: False, 1e-12: True})

    # the gather: exact ties of two columns (equal in A, c, g and hi)
    def tie(shape, pair, rel, rows, flagged=False):
        p, q = pair
        (r0, r1) = rows
        first = {0.0: (p, _var(shape, r1), 0), 1e-12: (p, _var(shape, r0), 0)}
        _add("cost-tau_tie@%d,%d-%s%s" % (p, q, shape, "-flagged" if flagged else ""), "cost", shape,
             functools.partial(cost_case, shape, pair, {r0: (1.0, Q, INF), r1: (1.0, Q_LO, INF)}, flagged=flagged),
             "tau", pair, rel, first, True, flagged=flagged)
    tie("TALL", (990, 1030), ("winner_wave15", "loser_wave0", "second_gather_step"), (30, 31))
    tie("TALL", (70, 1030), ("winner_not_wave15", "loser_wave0", "second_gather_step"), (30, 31))
    tie("TALL", (5, 1000), ("winner_not_wave15", "loser_wave15"), (30, 31))
    tie("WIDE", (1000, 2030), ("winner_wave15", "loser_wave15"), (3, 17))
    tie("WIDE", (2000, 3050), ("winner_wave15", "loser_wave15"), (3, 17))
    tie("WIDE", (2000, 3050), ("winner_wave15", "loser_wave15"), (3, 17), flagged=True)
    _add("cost-tau_lone@1010-TALL", "cost", "TALL",
         functools.partial(cost_case, "TALL", (1010,), {30: (1.0, Q, INF), 31: (1.0, Q_LO, INF)}, lone=True),
         "tau", (1010, None), ("lone_wave15",), {0.0: (1010, v(31), 0), 1e-12: (1010, v(30), 0)}, True)


_rhs_catalogue()
_cost_catalogue()
NAMES = tuple(CASES)
# where the crash runs (a reversed basis, a flagged slack) one reference walk takes over a second: the grid of such a
# case is split by eps into three tests, with every grid point kept
CRASHED = tuple(nm for nm in NAMES if CASES[nm].reverse or "slackup" in nm)
GRID_PARAMS = [(nm, (eps,)) for nm in NAMES if nm in CRASHED for eps in EPS] + [(nm, EPS) for nm in NAMES
                                                                                if nm not in CRASHED]
GRID_IDS = [nm + ("" if len(eps) > 1 else "-eps=%g" % eps[0]) for nm, eps in GRID_PARAMS]

# the eps and t_max edges of one `beyond` case per path: eps against |delta_r| = 8 (RHS) or |g_e| = 16 (cost), the
# pattern of the eps edges of bounded_parametric_large_cases.tall
EDGE_CASE = {"rhs": "rhs-beyond@1030,1031-TALL", "cost": "cost-beyond@1030,1031-TALL"}
EDGE_EPS = {"rhs": (np.nextafter(8.0, 0.0), 8.0), "cost": (np.nextafter(16.0, 0.0), 16.0)}
EDGE_TMAX = (0.0, TAU, np.nextafter(TAU, 1.0))
EDGE_BREAKS = 8


def ref(name, case, eps, max_breaks, t_max=INF):
    """The reference's result, computed once per (case, eps, max_breaks, t_max)."""
    return L.ref(("seam", name), CASES[name].path, case, eps=eps, max_breaks=max_breaks, t_max=t_max)
