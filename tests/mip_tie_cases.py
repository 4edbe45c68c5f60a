"""Inputs of the tests of the branch-and-bound node decisions at exact ties (inputs and memoised reference results, in
the style of tests/tallcases.py). The three searches (batched_mip.hip, batched_mip_bounded.hip and k_mipl_node of
mip_bounded_large.hip) decide at every node by comparisons that random data never lands on: the most fractional marked
column with an exact tie to the lowest index, dist against int_tol, f against 0.5, z against zstar +- gap. The cases
here land on them, across every seam of the three column scans: columns 64 apart share a lane of the two LDS kernels,
columns 1024 apart a thread of k_mipl_node, and between them lie the lanes of one wave (the __shfl_xor butterfly) and
the sixteen waves (k_mipl_node's LDS slots). tests/test_mip_ties_cpu.py shows on the references alone that each input
does what its name says, tests/test_gpu_mip_ties.py runs them on the GPU.

The gadget is separable: row i reads x_{p_i} + s_i = v_i, maximise with c_{p_i} > 0, marked columns in [0, 10], slacks
in [0, inf), started from the structural basis basis[i] = p_i without flags. Every x_{p_i} = v_i is basic at the root,
a down child is feasible (x = floor v), an up child is infeasible, so k fractional columns cost 2k + 1 nodes. All data
are small dyadic numbers. In a separable problem the order of branching changes neither x nor the node count, so the
order is read from the depth ladder: at max_depth = D the search abandons the node of level D and returns as `bound`
the root's z minus the drops f_j c_j of the first D columns branched on; the drops are chosen so that every set of D
columns has another sum.

Shapes:
  WIDE    24 x 4300  n_orig 4276: the HBM entry only; past one stride of k_mipl_node (1024) and one chunk of its
                     objective chain (4096)
  LDS16   64 x 192   n_orig 128: all three entries, the sixteen-wave instantiation of the LDS kernels
  LDS4    16 x 144   n_orig 128: the same columns in the four-wave instantiation
  SMALL    8 x 20    n_orig 12, column 11 continuous: the int_tol, direction and gap families and their batch
  TALL  1100 x 2200  n_orig 1100: the branching column at basis position 1030 (the recorded reference result)"""
import itertools
import json
import os
import types

import numpy as np

from tests import bounded_ref as B
from tests import mip_bounded_ref as R
from tests import mip_ref as M
from tests.mip_bounded_large_cases import pack, unpack   # noqa: F401 (pack: the fixture's maker)

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
INF = np.inf
WIDE, LDS16, LDS4, SMALL, TALL = (24, 4300), (64, 192), (16, 144), (8, 20), (1100, 2200)
N_ORIG = {WIDE: 4276, LDS16: 128, LDS4: 128, SMALL: 12, TALL: 1100}
HI = 10.0                 # the box of every marked column
FILL = (2.0, 1.0)         # (v, cost) of an integral row
Y = 11                    # SMALL's continuous column
DEEP = 64                 # the depth at which no ladder stops
TOL = 2.0 ** -20          # family B's int_tol
TOL_STEP = 2.0 ** -50     # TOL (1 + 2^-30) - TOL
TINY = 2.0 ** -40

# What lp_mip_bounded_fits and lp_mip_fits answer, as the largest max_depth each shape fits at (None: at no depth): the
# GPU test asserts them and lets nothing else decide which entries a case runs on.  The row form of batched_mip.hip
# grows by a row and a column per level and stops at 64.
BOUNDED_FITS_TO = {WIDE: None, LDS16: 185, LDS4: 1024, SMALL: 1024, TALL: None}
PLAIN_FITS_TO = {WIDE: None, LDS16: 22, LDS4: 64, SMALL: 64, TALL: None}


def fits(table, shape, depth):
    return table[shape] is not None and depth <= table[shape]


_CACHE = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _freeze(cs):
    for v in vars(cs).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def gadget(name, shape, cols, lo=None, flagged=(), unmarked=(), fill=FILL, fill_from=0, plain=True):
    """The separable problem: row i holds column cols[i] = (j, v, cost); the rows left over hold the lowest unused
    structural columns from fill_from on with fill = (v, cost).  lo: {j: lower bound} (0 elsewhere); flagged: basic
    columns started complemented (at_upper = 1); unmarked: structural columns that stay continuous.  plain: the rows
    without the boxes are the same problem (lo = 0 and no flag), so the case also runs on the row form."""
    m, n = shape
    no = N_ORIG[shape]
    assert n == no + m and len(cols) <= m
    used = {j for j, _, _ in cols}
    assert len(used) == len(cols) and all(0 <= j < no for j in used)
    rows = list(cols)
    j = fill_from
    while len(rows) < m:
        if j not in used:
            rows.append((j,) + tuple(fill))
        j += 1
    A, b, c = np.zeros((m, n)), np.zeros(m), np.zeros(n)
    lov, hiv = np.zeros(n), np.full(n, INF)
    hiv[:no] = HI
    mask = np.zeros(n, np.int32)
    mask[:no] = 1
    for j in unmarked:
        mask[j] = 0
        hiv[j] = INF
    for j, l in (lo or {}).items():
        lov[j] = l
    up = np.zeros(n, np.int32)
    basis = np.zeros(m, np.int32)
    for i, (j, v, cost) in enumerate(rows):
        A[i, j] = A[i, no + i] = 1.0
        b[i], c[j], basis[i] = v, cost, j
    for j in flagged:
        up[j] = 1
    frac = tuple((j, v, cost) for j, v, cost in rows if v != np.floor(v))
    return types.SimpleNamespace(name=name, shape=shape, n_orig=no, A=A, b=b, c=c, lo=lov, hi=hiv, basis=basis, up=up,
                                 mask=mask, maximize=True, rows=tuple(rows), frac=frac,
                                 plain=plain and not lo and not flagged)


def bounded_args(cs):
    return (cs.A, cs.b, cs.c, cs.lo, cs.hi, cs.basis, cs.up, cs.mask, cs.maximize, cs.n_orig)


def plain_args(cs):
    assert cs.plain
    return (cs.A, cs.b, cs.c, cs.basis, cs.mask, cs.maximize, cs.n_orig)


def _kw_key(kw):
    return tuple(sorted((k, float(v).hex() if isinstance(v, float) else v) for k, v in kw.items()))


def ref_bounded(cs, **kw):
    """mip_bounded_ref.mip of cs, once per (case name, limits) and never changed."""
    return _memo(("bounded", cs.name, _kw_key(kw)), lambda: R.mip(*bounded_args(cs), **kw))


def ref_plain(cs, **kw):
    """mip_ref.mip of the rows of cs without the boxes, once per (case name, limits)."""
    return _memo(("plain", cs.name, _kw_key(kw)), lambda: M.mip(*plain_args(cs), **kw))


# ---- what a case is designed to do, computed from its data alone (the CPU test holds the references against it) -----
def dist(v):
    f = v - np.floor(v)
    return f if f < 1.0 - f else 1.0 - f


def designed_order(cs, int_tol=1e-6):
    """The columns in the order the search must branch on them: the larger dist first, an exact tie to the lower
    index."""
    return tuple(j for j, v, _ in sorted(cs.frac, key=lambda r: (-dist(r[1]), r[0])) if dist(v) > int_tol)


def drop(cs, j):
    """What z loses when column j is branched to floor(v): f_j c_j (the up child is infeasible on either order)."""
    (v, cost), = [(v, cost) for q, v, cost in cs.frac if q == j]
    return (v - np.floor(v)) * cost


def root_z(cs):
    return float(sum(cost * v for _, v, cost in cs.rows))   # exact: small dyadic numbers


def ladder_bound(cs, cols):
    """The bound of a run that is abandoned after branching on `cols`."""
    return root_z(cs) - float(sum(drop(cs, j) for j in cols))


def other_sets(cs, depth, int_tol=1e-6):
    """Every set of `depth` fractional columns but the designed first `depth`."""
    order = designed_order(cs, int_tol)
    return [s for s in itertools.combinations(sorted(order), depth) if set(s) != set(order[:depth])]


def depths(cs):
    return tuple(range(1, len(cs.frac) + 1)) + (DEEP,)


def _with_drops(cols):
    """(j, v) -> (j, v, cost) with the drops f_j c_j = 2^-1, 2^-2, ... in the listed order: every set of columns has
    another sum.  f in {2^-1, .., 2^-7}, so the costs are powers of two as well."""
    out = []
    for i, (j, v) in enumerate(cols):
        f = v - np.floor(v)
        out.append((j, v, 2.0 ** -(i + 1) / f))
    return out


# ---- family A: the order of tied columns -----------------------------------------------------------------------------
# name -> ((j, v), ...) in cost order, the designed branching order.  k_mipl_node: thread j % 1024, wave
# (j % 1024) / 64.
WIDE_ORDER = {
    # 5, 1029 and 2053 share thread 5 (and 4101, past one chunk of products); 70 sits in wave 1; 4102 is thread 6, the
    # neighbouring lane of 4101's
    "wide_thread": (((5, 2.5), (1029, 2.5), (2053, 2.5), (70, 2.5), (4101, 4.5), (4102, 4.5)),
                    (5, 70, 1029, 2053, 4101, 4102)),
    # the lowest tied index in the LAST wave of a stride (thread 1000), the others in waves 0, 1 and 14: the walk over
    # the sixteen LDS slots decides, and it must not prefer the earlier wave
    "wide_last_wave": (((1027, 2.5), (2148, 4.5), (3000, 2.5), (1000, 2.5)), (1000, 1027, 2148, 3000)),
    # a tied pair of dist 0.25 at 10 and 74, a strictly larger dist behind it in thread 10 itself (1034) and in wave 14
    # (3000): larger wins over lower
    "wide_larger": (((10, 2.25), (74, 3.25), (1034, 2.5), (3000, 4.5)), (1034, 3000, 10, 74)),
}
# pairs (lower index, higher index) whose lanes differ in one bit, the LOWER index in the HIGHER lane: they meet at that
# offset of the butterfly, where `oj < jb` must carry the index over the lane.  Pair p has dist 2^-(p+1).
BUTTERFLY = ((32, 40, 8), (16, 20, 4), (8, 9, 1), (4, 38, 34), (2, 7, 5), (1, 61, 60))   # (offset, lane hi, lane lo)
SAME_LANE = (11, 75)      # j and j + 64: one lane of the LDS kernels


def _lane_pairs(stride, same_lane):
    pairs = [(hi_lane, stride + lo_lane) for _, hi_lane, lo_lane in BUTTERFLY]
    assert all(h ^ (l - stride) == off for (h, l), (off, _, _) in zip(pairs, BUTTERFLY))
    if same_lane:
        pairs.append(SAME_LANE)
    cols = []
    for p, (a, b) in enumerate(pairs):
        cols += [(b, 2.0 + 2.0 ** -(p + 1)), (a, 4.0 + 2.0 ** -(p + 1))]   # the higher index listed (and priced) first
    order = tuple(j for pair in pairs for j in pair)
    return tuple(cols), order


LDS_ORDER = {
    "lds_lanes": _lane_pairs(64, True),
    # six columns of dist 0.5: 11 and 75 share a lane, 40 / 72 and 20 / 68 meet at offsets 32 and 16
    "lds_equal": (((75, 2.5), (72, 4.5), (68, 2.5), (40, 2.5), (20, 4.5), (11, 2.5)), (11, 20, 40, 68, 72, 75)),
    # the tied pair (3, 67) of dist 0.25 in one lane, a strictly larger dist at 100 and 110
    "lds_larger": (((3, 2.25), (67, 3.25), (100, 2.5), (110, 4.5)), (100, 110, 3, 67)),
}
WIDE_ORDER["wide_lanes"] = _lane_pairs(1024, False)
ORDER_SHAPES = {**{name: (WIDE,) for name in WIDE_ORDER}, **{name: (LDS16, LDS4) for name in LDS_ORDER}}
ORDERS = {**WIDE_ORDER, **LDS_ORDER}
ORDER_CASES = tuple((name, shape) for name in ORDERS for shape in ORDER_SHAPES[name])


def order_case(name, shape):
    """Family A: the tied columns of ORDERS[name] at `shape`; .order is the designed branching order."""
    def make():
        cols, order = ORDERS[name]
        cs = gadget(f"{name}@{shape[0]}x{shape[1]}", shape, _with_drops(cols), fill_from=128 if shape == WIDE else 0)
        cs.order = order
        return _freeze(cs)
    return _memo(("order", name, shape), make)


# ---- family B: dist against int_tol ---------------------------------------------------------------------------------
# name -> (shape, the columns, their v, the limits, (status, found, stats, x of the columns) the reference must return).
# tol_zero: at int_tol = 0 the 2^-40 branches, and under the default eps = 1e-9 no child moves it (a bound violated by
# less than eps is none), so the search dives to the depth limit; at eps = 0 the first child rounds it away.
_EDGE, _BEYOND = (3.0 + TOL, 5.0 - TOL), (3.0 + TOL + TOL_STEP, 5.0 - TOL - TOL_STEP)
TOL_CASES = {
    "tol_edge": (SMALL, (2, 6), _EDGE, dict(int_tol=TOL), (OPTIMAL, 1, (1, 0, 0, 0, 0), _EDGE)),
    "tol_beyond": (SMALL, (2, 6), _BEYOND, dict(int_tol=TOL), (OPTIMAL, 1, (5, 2, 0, 0, 2), (3.0, 4.0))),
    "tol_zero": (SMALL, (2,), (3.0 + TINY,), dict(int_tol=0.0), (ITER_LIMIT, 0, (129, 0, 0, 0, 64), None)),
    "tol_zero_eps0": (SMALL, (2,), (3.0 + TINY,), dict(int_tol=0.0, eps=0.0), (OPTIMAL, 1, (3, 1, 0, 0, 1), (3.0,))),
    "wide_tol_edge": (WIDE, (1500, 3000), _EDGE, dict(int_tol=TOL), (OPTIMAL, 1, (1, 0, 0, 0, 0), _EDGE)),
    "wide_tol_beyond": (WIDE, (1500, 3000), _BEYOND, dict(int_tol=TOL), (OPTIMAL, 1, (5, 2, 0, 0, 2), (3.0, 4.0))),
}


def tol_case(name):
    def make():
        shape, cols, vs, kw, want = TOL_CASES[name]
        cs = gadget(name, shape, [(j, v, 1.0) for j, v in zip(cols, vs)], unmarked=(Y,) if shape == SMALL else (),
                    fill_from=128 if shape == WIDE else 0)
        cs.kw, cs.want = dict(kw, max_depth=DEEP), want
        return _freeze(cs)
    return _memo(("tol", name), make)


# ---- family C: f against 0.5, floor and ceil of negative values, flagged basic columns -------------------------------
DIR_COLS = {
    # 2.5 and 4.5: f = 0.5 exactly, down first; 2.75: up first, the dive ends INFEASIBLE; 3.25: down first
    "dir_pos": ((1, 2.5), (4, 4.5), (7, 2.75), (9, 3.25)),
    # with lo = -5 on columns 3 and 10: floor(-2.5) = -3 and f = 0.5, down first; f(-2.25) = 0.75, up first
    "dir_neg": ((1, 2.5), (3, -2.5), (4, 4.5), (7, 2.75), (9, 3.25), (10, -2.25)),
    "dir_flagged": ((1, 2.5), (3, -2.5), (4, 4.5), (7, 2.75), (9, 3.25), (10, -2.25)),
    "half": ((5, 2.5),),
    "half_above": ((5, 2.5 + 2.0 ** -30),),
}
DIR_LO = {"dir_neg": {3: -5.0, 10: -5.0}, "dir_flagged": {3: -5.0, 10: -5.0}}
DIR_FLAGGED = {"dir_flagged": (1, 3, 7)}     # started complemented: the `if (f)` arms of the dive
DIR_ORDER = {"dir_pos": (1, 4, 7, 9), "dir_neg": (1, 3, 4, 7, 9, 10), "dir_flagged": (1, 3, 4, 7, 9, 10),
             "half": (5,), "half_above": (5,)}
DIR_UP_FIRST = {"dir_pos": 1, "dir_neg": 2, "dir_flagged": 2, "half": 0, "half_above": 1}   # dives that end INFEASIBLE


def dir_case(name):
    def make():
        cols = [(j, v, 4.0 ** -i) for i, (j, v) in enumerate(DIR_COLS[name])]   # drops f 4^-i, f in {1/4, 1/2, 3/4}
        cs = gadget(name, SMALL, cols, lo=DIR_LO.get(name), flagged=DIR_FLAGGED.get(name, ()), unmarked=(Y,))
        cs.order = DIR_ORDER[name]
        return _freeze(cs)
    return _memo(("dir", name), make)


def node_limits(cs):
    return tuple(range(1, 2 * len(cs.frac) + 2))


# ---- family D: z against zstar +- gap --------------------------------------------------------------------------------
GAP_EDGE = 0.25
GAPS = (GAP_EDGE, GAP_EDGE + TINY, GAP_EDGE - TINY)
LIMIT_EDGE = 0.5          # root z - incumbent: the node-limit form
LIMIT_GAPS = (LIMIT_EDGE, LIMIT_EDGE + TINY, LIMIT_EDGE - TINY)
GAP_XY = {SMALL: (3, Y), WIDE: (2000, 4275)}


def gap_case(shape, maximize, y_marked=False):
    """Row 0: x - y + s = 2.5 with x integer in [0, 10], y >= 0, c = (1, -1.5, 0), beside integral rows; min: c
    negated.  The root is bounded_ref.bounded's.  The down child is the incumbent 2 (+ K of the other rows), the up
    child is feasible at x = 3, y = 0.5, z = 2.25 (+ K).  y_marked: y is an integer column too, so that the 2.25 node
    is fractional and at max_depth = 1 abandoned."""
    def make():
        xj, yj = GAP_XY[shape]
        tag = ("max" if maximize else "min") + ("_depth" if y_marked else "")
        cs = gadget(f"gap_{tag}@{shape[0]}x{shape[1]}", shape, [(xj, 2.5, 1.0)], unmarked=() if y_marked else (yj,),
                    fill_from=128 if shape == WIDE else 0)
        cs.hi[yj] = INF
        cs.A[0, yj] = -1.0
        cs.c[yj] = -1.5
        if not maximize:
            cs.c *= -1.0
            cs.maximize = False
        cs.structural = cs.basis
        root = B.bounded(cs.A, cs.b, cs.c, cs.lo, cs.hi, cs.maximize)
        cs.root_status, cs.basis, cs.up = root["status"], root["basis"], root["at_upper"]
        cs.x, cs.y = xj, yj
        cs.K = float(sum(cost * v for _, v, cost in cs.rows[1:]))
        return _freeze(cs)
    return _memo(("gap", shape, maximize, y_marked), make)


TWIN_XY = ((3, 10), (4, 11))     # two blocks at SMALL: (x, y) of rows 0 and 1, every column marked
TWIN_RUN = dict(max_depth=2)
TWIN_WANT = (ITER_LIMIT, 1, (7, 6, 0, 0, 2), 4.0, 4.5)   # status, found, stats, obj - K, bound - K


def gap_twin_case():
    """Two blocks x - y + s = 2.5 with both y integer, max_depth = 2: the nodes (x1, x2) = (2, 3) and (3, 2) are both
    fractional at the depth limit with z = 4.25 (+ K), so the second is compared with the first abandoned z at gap = 0
    on equal values; (3, 3) at 4.5 then replaces it.  (Either outcome of the comparison on equal values stores the same
    bits: the case runs it, no output tells the outcomes apart.)"""
    def make():
        cs = gadget("gap_twin", SMALL, [(x, 2.5, 1.0) for x, _ in TWIN_XY])
        for i, (_, yj) in enumerate(TWIN_XY):
            cs.hi[yj] = INF
            cs.A[i, yj] = -1.0
            cs.c[yj] = -1.5
        cs.K = float(sum(cost * v for _, v, cost in cs.rows[2:]))
        return _freeze(cs)
    return _memo(("gap_twin",), make)


# ---- family E: the objective chain across 4096 products --------------------------------------------------------------
BIG = 2.0 ** 57
# zero columns with costs, non-basic: (j, lo, hi, at_upper, cost); 8 * 2^57 enters the chain before 4096, leaves behind
CHAIN_COLS = ((4090, 0.0, 8.0, 1, BIG), (4094, 0.0, 1.0, 1, 0.375), (4100, 8.0, 10.0, 0, -BIG))


def chain_case():
    def make():
        cols, order = WIDE_ORDER["wide_thread"]
        cs = gadget("wide_chain", WIDE, _with_drops(cols), fill_from=128, plain=False)
        cs.order = order
        for j, l, h, f, cost in CHAIN_COLS:
            cs.lo[j], cs.hi[j], cs.up[j], cs.c[j] = l, h, f, cost
        return _freeze(cs)
    return _memo(("chain",), make)


def chain_sums(cs, x):
    """c.x of the full vertex x three ways: one serial chain in index order (the reference), one chain per 4096 products
    added up, and exactly."""
    from fractions import Fraction
    prod = cs.c * x
    serial = 0.0
    for p in prod:
        serial += p
    chunked = 0.0
    for base in range(0, len(prod), 4096):
        part = 0.0
        for p in prod[base:base + 4096]:
            part += p
        chunked += part
    exact = float(sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(cs.c, x)))
    return float(serial), float(chunked), exact


# ---- family F: the branching column at a basis position >= 1024 ------------------------------------------------------
TALL_COLS = ((1030, 2.5, 0.5), (1090, 4.5, 0.25), (7, 1.25, 0.125))
TALL_FILL = (3.0, 1.0)
TALL_RUN = dict(max_depth=1)
TALL_WANT = (ITER_LIMIT, 3293.28125, (3, 1, 0, 0, 1))     # status, bound, stats
TALL_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mip_ties_tall.json")


def tall_case():
    """p_i = i: column j is basic at position j, so the first branching column, 1030, is found by the second step of the
    scan strided by 1024."""
    def make():
        m = TALL[0]
        val = {j: (v, cost) for j, v, cost in TALL_COLS}
        cs = gadget("tall_position", TALL, [(i,) + val.get(i, TALL_FILL) for i in range(m)], plain=False)
        return _freeze(cs)
    return _memo(("tall",), make)


def tall_fixture():
    """The reference's recorded result of tall_case() under TALL_RUN (about 6 s on one core, so it is not recomputed in
    the GPU test)."""
    with open(TALL_FIXTURE) as f:
        return unpack(json.load(f)["result"])


# ---- the batch: families B to D at 8 x 20 under one mask -------------------------------------------------------------
BATCH_KW = dict(int_tol=TOL, gap=GAP_EDGE, max_depth=DEEP)


def batch_cases(plain):
    """The 8 x 20 cases that share SMALL's mask and the maximising sense, for one launch: neighbouring workgroups take
    different decisions.  plain: those that also run on the row form."""
    cs = [tol_case("tol_edge"), tol_case("tol_beyond"), dir_case("dir_pos"), dir_case("dir_neg"),
          dir_case("dir_flagged"), gap_case(SMALL, True), dir_case("half"), dir_case("half_above")]
    return [c for c in cs if c.plain] if plain else cs

