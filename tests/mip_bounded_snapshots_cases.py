"""The inputs that tests/test_mip_bounded_snapshots_cpu.py and tests/test_gpu_mip_bounded_snapshots.py share, and their
reference results (tests/ref/mip_bounded_snapshots_ref.c through tests/mip_bounded_snapshots_ref.py), computed once per
key and never changed.  The larger problems are tests/mip_bounded_large_cases.py's.  Test infrastructure only."""
import functools
import json
import os

import numpy as np

from tests import mip_bounded_large_cases as Q
from tests import mip_bounded_ref as R
from tests import mip_bounded_snapshots_ref as S

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)

# R.boxed_knapsack(seed, 4, 10): 4 x 14, tens of nodes.  Under KNAP_KW with 3 snapshots the reference returns
# seed -> (nodes, restores, rebuilds, restored children that end INFEASIBLE)
KNAP_KW = dict(max_depth=24, max_nodes=400)
KNAP_AT_3 = {1: (83, 22, 19, 11), 2: (79, 29, 10, 3), 5: (77, 23, 15, 9), 6: (79, 23, 16, 2)}
KNAP_KS = (1, 3, 24)

# 160 x 320 "mixed" seed 3, min, 60 nodes, depth 64: K -> (restores, rebuilds)
MIXED_3_MIN = {4: (15, 6), 64: (21, 0)}
# the BOX_SEEDS runs at max_depth 8 with 3 snapshots, each seed: (restores, rebuilds)
BOX_AT_3 = (25, 3)
# Q.BEYOND_INFEASIBLE_DIVES with 3 snapshots: (restores, rebuilds, restored children that end INFEASIBLE)
INFEASIBLE_DIVES_AT_3 = (6, 1, 1)

BEYOND_SEEDS = (1, 3)
KS_67 = (2, 64)
KS_160 = (4, 64)
LDS_BOX = (32, 96, 256, "box")   # Q.LDS_SHAPES[1]
KS_LDS_BOX = (4, 256)

TALL_DEPTH, TALL_NODES, TALL_SNAPSHOTS = 2, 6, 2
TALL_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mip_bounded_snapshots_tall.json")

_ref_cache = {}


def ref(key, args, **kw):
    """S.mip(*args, **kw) (kw with snapshots), computed once per (key, kw)."""
    full = (key, tuple(sorted(kw.items())))
    if full not in _ref_cache:
        _ref_cache[full] = S.mip(*args, **kw)
    return _ref_cache[full]


@functools.lru_cache(maxsize=None)
def knapsack_args(seed):
    A, b, c, lo, hi, mask, root = R.boxed_knapsack(seed, 4, 10)
    assert root["status"] == OPTIMAL and A.shape == (4, 14)
    return Q._freeze([A, b, c, lo, hi, root["basis"], root["at_upper"], mask]) + (True, 10)


def large_cases():
    """Every search of mip_bounded_large_cases: (key, args, kw) with kw = max_depth and max_nodes."""
    for m, n, depth, kind in Q.LDS_SHAPES:
        for mx in (True, False):
            for seed in range(3):
                for every in (1, 2):
                    kw = dict(max_depth=depth, max_nodes=Q.LDS_NODES)
                    got = Q.searched(m, n, seed, mx, kind, every, **kw)
                    if got is not None:
                        yield (m, n, seed, mx, kind, every), got[0], kw
    for m, n, seed, mx, nodes in Q.BEYOND:
        kw = dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes)
        yield (m, n, seed, mx, "mixed", 2), Q.searched(m, n, seed, mx, "mixed", 2, **kw)[0], kw
    m, n, seed, mx, every, nodes = Q.BEYOND_INFEASIBLE_DIVES
    kw = dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes)
    yield (m, n, seed, mx, "mixed", every), Q.searched(m, n, seed, mx, "mixed", every, **kw)[0], kw
    for seed in Q.BOX_SEEDS:
        for depth in (8, 64):
            kw = dict(max_depth=depth, max_nodes=60)
            yield (160, 320, seed, True, "box", 1), Q.searched(160, 320, seed, True, "box", 1, **kw)[0], kw


def gpu_keys():
    """The searches tests/test_gpu_mip_bounded_snapshots.py compares at K > 0 beyond the knapsacks, nothing computed:
    (key, kw, Ks) with key the arguments of Q.searched."""
    out = []
    for m, n, Ks in ((67, 201, KS_67), (160, 320, KS_160)):
        for seed in BEYOND_SEEDS:
            for mx in (True, False):
                out.append(((m, n, seed, mx, "mixed", 2), dict(max_depth=Q.BEYOND_DEPTH, max_nodes=60), Ks))
    m, n, seed, mx, every, nodes = Q.BEYOND_INFEASIBLE_DIVES
    out.append(((m, n, seed, mx, "mixed", every), dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes), (3,)))
    for seed in Q.BOX_SEEDS:
        out.append(((160, 320, seed, True, "box", 1), dict(max_depth=8, max_nodes=60), (3,)))
    return out


def gpu_cases():
    """gpu_keys() with the arguments: (key, args, kw, Ks)."""
    for key, kw, Ks in gpu_keys():
        yield key, Q.searched(*key, **kw)[0], kw, Ks


@functools.lru_cache(maxsize=None)
def stop_points(seed=1, snapshots=3):
    """Node budgets at which the search of knapsack_args(seed) stops in each way: dict(branching=N, second=N,
    restore=N), the smallest N >= 2 of each kind.  The node after the N-th is a first child (the search with
    max_nodes = N stops on a branching node, after the record and before any snapshot), a second child (it stops before
    a second child), or a second child that would have been restored."""
    args = knapsack_args(seed)
    total = ref(("knap", seed), args, snapshots=snapshots, **KNAP_KW)["stats"][0]
    out = {}
    prev = ref(("knap", seed), args, snapshots=snapshots, max_depth=KNAP_KW["max_depth"], max_nodes=2)
    for N in range(2, total):
        nxt = ref(("knap", seed), args, snapshots=snapshots, max_depth=KNAP_KW["max_depth"], max_nodes=N + 1)
        assert prev["status"] == ITER_LIMIT and prev["stats"][0] == N
        restored, rebuilt = nxt["stats"][5] - prev["stats"][5], nxt["stats"][6] - prev["stats"][6]
        kind = "restore" if restored else "second" if rebuilt else "branching"
        out.setdefault(kind, N)
        if restored:
            out.setdefault("second", N)
        prev = nxt
    return out


def iter_limit_case():
    """One row, x0 + x1 = 2.6, max x0, x0 integer in [0, 3], x1 in [0, 1], from the basis {x0}: the root is x0 = 2.6;
    the first child (up, x0 >= 3) leaves x1 = -0.4 with no column to enter, LP_INFEASIBLE without a pivot; the second
    child (x0 <= 2) needs one dual pivot, so under max_iter = 1 it ends LP_ITER_LIMIT, whether restored or rebuilt."""
    A = np.array([[1.0, 1.0]])
    args = (A, np.array([2.6]), np.array([1.0, 0.0]), np.zeros(2), np.array([3.0, 1.0]), np.array([0], np.int32),
            np.zeros(2, np.int32), np.array([1, 0], np.int32), True, 2)
    return args, dict(max_depth=8, max_nodes=50, max_iter=1)


def tall_fixture():
    """The reference's recorded result for Q.tall_args(1) at TALL_DEPTH, TALL_NODES, TALL_SNAPSHOTS."""
    with open(TALL_FIXTURE) as f:
        data = json.load(f)
    return Q.unpack(data["result"]), data
