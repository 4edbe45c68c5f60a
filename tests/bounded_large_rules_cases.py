"""The inputs that tests/test_bounded_large_rules_cpu.py and tests/test_gpu_bounded_large_rules.py share (those of
tests/bounded_large_cases.py and tests/bounded_resolve_large_cases.py plus the cycling LPs of tests/bounded_rules_ref.py),
what the rules reference (tests/ref/bounded_rules_ref.c, tests/ref/bounded_resolve_rules_ref.c) counts on them, and
its results, computed once per key and never changed.  Test infrastructure only."""
import functools

import numpy as np

from tests import bounded_large_cases as K
from tests import bounded_resolve_large_cases as Q
from tests import bounded_rules_ref as RR

INF = np.inf
OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
DANTZIG, BLAND, DEVEX = RR.RULES
NEW_RULES = (BLAND, DEVEX)
RULE_NAMES = {DANTZIG: "dantzig", BLAND: "bland", DEVEX: "devex"}

# (m, n, kind, seed) of K.boxed -> {rule: (status, [phase-I pivots, drive-out pivots, phase-II pivots, flips])}
BOXED = {
    (67, 201, "mixed", 1): {DANTZIG: (OPTIMAL, [374, 0, 103, 198]), BLAND: (OPTIMAL, [2194, 0, 553, 1456]),
                            DEVEX: (OPTIMAL, [92, 0, 78, 64])},
    (160, 320, "mixed", 1): {DANTZIG: (OPTIMAL, [930, 0, 208, 475]), BLAND: (OPTIMAL, [6019, 0, 1634, 4426]),
                             DEVEX: (OPTIMAL, [195, 0, 126, 77])},
    (160, 320, "box", 1): {BLAND: (OPTIMAL, [7408, 0, 1459, 135]), DEVEX: (OPTIMAL, [191, 0, 124, 96])},
    (160, 320, "unbounded", 1): {BLAND: (UNBOUNDED, [5907, 0, 70, 3344]), DEVEX: (UNBOUNDED, [206, 0, 34, 32])},
    (200, 500, "mixed", 1): {DEVEX: (OPTIMAL, [250, 0, 285, 183])},
}
BOXED_CASES = [(key, rule) for key in BOXED for rule in NEW_RULES if rule in BOXED[key]]
BOXED_MAX_ITER = 10000

# more rows than the selectors have threads (and more columns than one tile of Bland's first-hit scan)
TALL_SHAPE = K.TALL_SHAPE
TALL_MAX_ITER = K.TALL_MAX_ITER
TALL = {BLAND: (ITER_LIMIT, [69, 0, 0, 81]), DEVEX: (ITER_LIMIT, [82, 0, 0, 68])}
# more columns than one step of Devex's pricing and staging loops (4 x 1024): K.boxed(24, 4300, "mixed", 1), whose
# optimal basis holds columns beyond 4096 under every rule
WIDE_KEY = (24, 4300, "mixed", 1)
WIDE = {DANTZIG: (OPTIMAL, [30, 0, 128, 342]), BLAND: (OPTIMAL, [326, 0, 2099, 6825]),
        DEVEX: (OPTIMAL, [32, 0, 127, 322])}

# RR.cycling_boxed(), maximise, max_iter = 5000; RR.beale_boxed(), maximise, max_iter = 1000
CYCLING_MAX_ITER = 5000
CYCLING = {DANTZIG: (ITER_LIMIT, [105, 0, 5000, 0]), BLAND: (OPTIMAL, [439, 0, 82, 0]), DEVEX: (OPTIMAL, [77, 0, 33, 0])}
BEALE_MAX_ITER = 1000
BEALE = {DANTZIG: (ITER_LIMIT, None), BLAND: (OPTIMAL, [3, 0, 2, 0])}

# K.driveout_with_flip keys -> {rule: iters}
DRIVEOUT_FLIP = {
    (8, 16, 4, 223, 3): {BLAND: [18, 2, 4, 1], DEVEX: [8, 0, 3, 1]},
    (8, 16, 4, 677, 0): {BLAND: [13, 2, 4, 0], DEVEX: [16, 1, 1, 0]},
    (16, 30, 8, 1979, 4): {BLAND: [63, 2, 1, 0], DEVEX: [27, 1, 2, 1]},
    (16, 30, 8, 2197, 5): {BLAND: [38, 1, 13, 0], DEVEX: [23, 0, 1, 0]},
}
# K.driveout(seed): Bland ends optimal after 5 to 7 drive-out pivots; Devex is no anti-cycling rule and cycles there,
# so it runs to this limit
DRIVEOUT_SEEDS = (5, 6, 7, 8)
DRIVEOUT_DEVEX_MAX_ITER = 500

# the sweep of max_iter on boxed(160, 320, "mixed", 1) under Devex: the first iterations mix flips and pivots
LIMIT_SWEEP = (1, 2, 50, 51)

# the re-solve: name -> {rule: [dual pivots, primal pivots, flips]}
RESOLVE = {
    "cost_max": {DANTZIG: [0, 15, 3], BLAND: [0, 18, 26], DEVEX: [0, 11, 4]},
    "cost_min": {DANTZIG: [0, 5, 9], BLAND: [0, 12, 14], DEVEX: [0, 5, 5]},
    "unit_costs": {DANTZIG: [0, 379, 0], BLAND: [0, 3641, 0], DEVEX: [0, 285, 0]},
    "unit_costs_reversed": {DANTZIG: [0, 379, 0], BLAND: [0, 3641, 0], DEVEX: [0, 285, 0]},
    "bound_max": {DANTZIG: [41, 0, 0], BLAND: [41, 0, 0], DEVEX: [41, 0, 0]},   # the dual branch
}


@functools.lru_cache(maxsize=None)
def resolve_start(name):
    """(warm start, maximize) of the re-solve case `name`; the cold solves are the Dantzig reference's."""
    if name.startswith("unit_costs"):
        return Q.unit_costs(1, name.endswith("reversed")), True
    kind, sense = name.split("_")
    maximize = sense == "max"
    return Q.warm(160, 320, 1, maximize, kind, Q.cold_ref(160, 320, 1, maximize)), maximize


@functools.lru_cache(maxsize=None)
def lds_warm_starts(m, n, seed, maximize):
    """The warm starts of tests/test_gpu_bounded_resolve_large.py at a shape that fits LDS: [(kind, start)], empty when
    the cold solve is not optimal."""
    from tests import bounded_resolve_ref as W
    cold = Q.cold_ref(m, n, seed, maximize)
    if cold["status"] != OPTIMAL:
        return []
    return [(kind, Q.warm(m, n, seed, maximize, kind, cold)) for kind in W.PERTURBATIONS]


_ref_cache = {}


def ref(key, rule, A, b, c, lo, hi, maximize, n_orig=None, eps=1e-9, max_iter=10000):
    """RR.bounded(..., rule=rule), computed once per (key, rule)."""
    if (key, rule) not in _ref_cache:
        _ref_cache[(key, rule)] = RR.bounded(A, b, c, lo, hi, maximize, n_orig, eps, max_iter, rule)
    return _ref_cache[(key, rule)]


def resolve_ref(key, rule, start, maximize, n_orig=None, eps=1e-9, max_iter=10000):
    """RR.resolve(*start, ..., rule=rule), computed once per (key, rule)."""
    if ("resolve", key, rule) not in _ref_cache:
        _ref_cache[("resolve", key, rule)] = RR.resolve(*start, maximize, n_orig, eps, max_iter, rule)
    return _ref_cache[("resolve", key, rule)]


def boxed_ref(key, rule):
    m, n, kind, seed = key
    A, b, c, lo, hi, mx = K.boxed(*key)
    return ref(("boxed",) + key, rule, A, b, c, lo, hi, mx, n - m, max_iter=BOXED_MAX_ITER)


def tall_ref(rule):
    m, n = TALL_SHAPE
    A, b, c, lo, hi, mx = K.boxed(m, n, "mixed", 1)
    return ref("tall", rule, A, b, c, lo, hi, mx, n - m, max_iter=TALL_MAX_ITER)


def wide_ref(rule):
    m, n = WIDE_KEY[:2]
    A, b, c, lo, hi, mx = K.boxed(*WIDE_KEY)
    return ref("wide", rule, A, b, c, lo, hi, mx, n - m)


def cycling_ref(rule):
    return ref("cycling", rule, *RR.cycling_boxed(), True, max_iter=CYCLING_MAX_ITER)


def beale_ref(rule):
    return ref("beale", rule, *RR.beale_boxed(), True, max_iter=BEALE_MAX_ITER)


def driveout_ref(seed, rule):
    A, b, c, lo, hi, mx = K.driveout(seed)
    return ref(("driveout", seed), rule, A, b, c, lo, hi, mx,
               max_iter=DRIVEOUT_DEVEX_MAX_ITER if rule == DEVEX else 10000)


def driveout_flip_ref(key, rule):
    return ref(("driveout_flip",) + key, rule, *K.driveout_with_flip(*key))
