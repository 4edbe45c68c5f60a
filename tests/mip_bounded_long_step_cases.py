"""The inputs that tests/test_mip_bounded_long_step_cpu.py and tests/test_gpu_mip_bounded_long_step.py share, and their
reference results (tests/ref/mip_bounded_long_step_ref.c through tests/mip_bounded_long_step_ref.py), computed once per
key and never changed.  Every problem comes from an existing generator: mip_bounded_ref.boxed_mip (through
mip_bounded_large_cases.problem), mip_bounded_large_cases, mip_bounded_snapshots_cases, mip_ref.knapsack and
bounded_resolve_ref.perturb.  Test infrastructure only."""
import functools

import numpy as np

from tests import bounded_ref as B
from tests import bounded_resolve_ref as BR
from tests import mip_bounded_large_cases as Q
from tests import mip_bounded_long_step_ref as L
from tests import mip_bounded_ref as R
from tests import mip_bounded_snapshots_cases as SC
from tests import mip_ref as M

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
TEXTBOOK, LONG_STEP = L.TEXTBOOK, L.LONG_STEP

# (m, n, max_depth, kind): the shapes of test_gpu_mip_bounded.py's shape test; 65 x 193 > 4096 cells runs the
# 1024-thread block, the others the 256-thread one
LDS_SHAPES = [(4, 10, 16, "mixed"), (8, 20, 32, "mixed"), (16, 40, 64, "box"), (32, 96, 256, "box"),
              (64, 192, 64, "box")]
LDS_SEEDS = (0, 1, 2)
LDS_NODES = 150
LDS_KS = (0, 2)   # the HBM entry at these shapes: these and max_depth

# Q.BEYOND at its node limits: 67 x 201 (an odd row length, 202 columns padded to 208 in HBM; it also fits LDS at this
# depth) and 160 x 320 (beyond the LDS fit)
BEYOND_SHAPES = ((67, 201), (160, 320))
BEYOND_KS = (0, 4)
# the rebuild-heavy box case of Q.BOX_SEEDS: max_depth 8, 60 nodes
BOX_KEY, BOX_KW = (160, 320, 1, True, "box", 1), dict(max_depth=8, max_nodes=60)

_ref_cache = {}


def ref(key, args, **kw):
    """L.mip(*args, **kw) (kw with snapshots and dual_ratio), computed once per (key, kw)."""
    full = (key, tuple(sorted(kw.items())))
    if full not in _ref_cache:
        _ref_cache[full] = L.mip(*args, **kw)
    return _ref_cache[full]


def lds_keys():
    """(key, kw) of every search at the LDS shapes, nothing computed: key the arguments of Q.problem."""
    return [((m, n, seed, mx, kind, 1), dict(max_depth=depth, max_nodes=LDS_NODES))
            for m, n, depth, kind in LDS_SHAPES for mx in (True, False) for seed in LDS_SEEDS]


def args_of(key):
    """The arguments of ctx.mip_bounded_solve for Q.problem(*key), or None when its cold root is not optimal."""
    m, n = key[0], key[1]
    A, b, c, lo, hi, mask, root = Q.problem(*key)
    if root["status"] != OPTIMAL:
        return None
    return (A, b, c, lo, hi, root["basis"], root["at_upper"], mask, key[3], n - m)


def beyond_keys():
    """(key, kw) of the HBM entry's own searches: Q.BEYOND's 67 x 201 and 160 x 320 problems at their node limits,
    then the max_depth-8 box case."""
    out = [((m, n, seed, mx, "mixed", 2), dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes))
           for m, n, seed, mx, nodes in Q.BEYOND if (m, n) in BEYOND_SHAPES]
    return out + [(BOX_KEY, dict(BOX_KW))]


@functools.lru_cache(maxsize=None)
def root_after_bound_change(m=8, n=20, kind="mixed"):
    """A root whose own dual loop flips: the first Q.problem(m, n, seed, True, kind, 1) and perturbation
    (bounded_resolve_ref.perturb, "bound": one to three bounds of basic columns tightened, the marked columns' bounds
    then rounded inward to integers so that the old vertex stays cut off) whose root, by the reference under
    LONG_STEP, ends optimal after at least one flip of its own and is then searched.  Returns (key, args, kw)."""
    kw = dict(max_depth=32, max_nodes=LDS_NODES)
    for seed in range(40):
        A, b, c, lo, hi, mask, root = Q.problem(m, n, seed, True, kind, 1)
        if root["status"] != OPTIMAL:
            continue
        full = B.bounded(A, b, c, lo, hi, True, n)["x"]
        for pseed in range(12):
            _, _, lo2, hi2 = BR.perturb(pseed, "bound", b, c, lo, hi, root["basis"], full)
            for j in np.flatnonzero(mask):
                lo2[j] = np.ceil(lo2[j])
                if np.isfinite(hi2[j]):
                    hi2[j] = np.floor(hi2[j])
            args = (A, b, c, lo2, hi2, root["basis"], root["at_upper"], mask, True, n - m)
            key = ("root", m, n, seed, pseed)
            r = ref(key, args, dual_ratio=LONG_STEP, **kw)
            if r["diag"]["flips_root"] > 0 and r["stats"][0] > 1 and r["status"] in (OPTIMAL, ITER_LIMIT):
                return key, Q._freeze(list(args[:8])) + args[8:], kw
    raise AssertionError("no root whose dual loop flips")


@functools.lru_cache(maxsize=None)
def outcome_cases():
    """test_gpu_mip_bounded._outcome_cases built on the long-step reference: its five fixed problems, and the four
    kinds its seed scan looks for (optimal, node_limit, depth_limit, iter_limit) found with LONG_STEP under the same
    limits.  Returns (A, b, c, lo, hi, basis, at_upper (each stacked), mask, kinds, limits, expect)."""
    from tests.test_gpu_mip_bounded import _outcome_cases, _stack
    A, b, c, lo, hi, basis, up, mask, kinds, kw, expect = _outcome_cases()
    fixed = ("integer_infeasible", "unbounded_root", "singular_start", "no_valid_start", "crossed_bounds")
    cases = {k: tuple(v[kinds.index(k)] for v in (A, b, c, lo, hi, basis, up)) for k in fixed}
    zero, none = np.zeros(7), np.zeros(7, np.int32)
    box = np.r_[np.full(4, 4.0), np.full(3, np.inf)]
    want = ("optimal", "node_limit", "depth_limit", "iter_limit")
    for s in range(4000):
        if all(k in cases for k in want):
            break
        A1, b1, c1, bs, _ = M.knapsack(7000 + s, 3, 4, box=4)
        r = L.mip(A1, b1, c1, zero, box, bs, none, mask, True, 4, dual_ratio=LONG_STEP, **kw)
        st, nodes = r["status"], r["stats"][0]
        if st == OPTIMAL and nodes > 1:
            kind = "optimal"
        elif st == ITER_LIMIT and nodes == kw["max_nodes"]:
            kind = "node_limit"
        elif st == ITER_LIMIT and nodes == 1:
            kind = "iter_limit"
        elif st == ITER_LIMIT and r["found"] and r["bound"] > r["obj"] and r["stats"][4] == kw["max_depth"]:
            kind = "depth_limit"
        else:
            continue
        cases.setdefault(kind, (A1, b1, c1, zero, box, bs, none))
    names = sorted(cases)
    return tuple(_stack([cases[k] for k in names])) + (mask, names, kw, expect)


@functools.lru_cache(maxsize=None)
def node_at_max_iter():
    """A search that a node's dual loop stops at max_iter after the root: SC.iter_limit_case (its second child needs
    one dual pivot under max_iter = 1), and the first LDS case whose search under max_iter = 2 is stopped by a dual
    loop that has flipped.  Returns [(key, args, kw)]."""
    args, kw = SC.iter_limit_case()
    out = [(("iter_limit_case",), args, kw)]
    for key, kw2 in lds_keys():
        a = args_of(key)
        if a is None or key[0] > 16:
            continue
        kw3 = dict(kw2, max_iter=2)
        r = ref(key, a, dual_ratio=LONG_STEP, snapshots=0, **kw3)
        if r["status"] == ITER_LIMIT and r["diag"]["dual_iter_limit"] == 1 and r["stats"][3] > 0 and r["stats"][0] > 1 \
                and r["stats"][0] < kw3["max_nodes"]:
            out.append((key, a, kw3))
            break
    return out


@functools.lru_cache(maxsize=None)
def batch_of_64(m=16, n=40, Bn=64):
    """64 box problems of 16 x 40 with one mask and their cold roots: (A, b, c, lo, hi (stacked), mask, basis,
    at_upper, status), the limits."""
    cases = [Q.problem(m, n, 200 + k, True, "box", 1) for k in range(Bn)]
    A, b, c, lo, hi = (np.stack([cs[i] for cs in cases]) for i in range(5))
    root = [cs[6] for cs in cases]
    ok = np.array([r["status"] == OPTIMAL for r in root])
    basis = np.stack([np.asarray(r["basis"], np.int32) if o else np.zeros(m, np.int32) for r, o in zip(root, ok)])
    up = np.stack([np.asarray(r["at_upper"], np.int32) if o else np.zeros(n, np.int32) for r, o in zip(root, ok)])
    status = np.array([r["status"] for r in root], np.int32)
    return (A, b, c, lo, hi, cases[0][5], basis, up, status), dict(max_depth=64, max_nodes=40)


def deep_args():
    """R.deep_case() as the arguments of ctx.mip_bounded_solve and the limits."""
    A, b, c, lo, hi, mask, maximize, root = R.deep_case()
    return (A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, R.DEEP_K), dict(max_depth=1024)
