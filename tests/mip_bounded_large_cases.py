"""The inputs that tests/test_mip_bounded_large_cpu.py and tests/test_gpu_mip_bounded_large.py share, and their
reference results (tests/ref/mip_bounded_ref.c through tests/mip_bounded_ref.py), computed once per key and never
changed.  A problem is (A, b, c, lo, hi, mask, maximize) with its root by bounded_ref.bounded.  Test infrastructure
only."""
import functools
import json
import os

import numpy as np

from tests import bounded_ref as B
from tests import mip_bounded_ref as R

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)

# shapes lp_mip_bounded_fits accepts at these depths: (m, n, max_depth, kind), as test_gpu_mip_bounded.py's shape test
LDS_SHAPES = [(8, 20, 32, "mixed"), (32, 96, 256, "box"), (64, 192, 64, "box")]
LDS_NODES = 150

# beyond the fit: boxed_mip(seed, m, n, maximize, "mixed", 2) -> (m, n, seed, maximize, max_nodes); 67 x 201 is here
# for its odd row length (202 columns padded to 208)
BEYOND = ([(160, 320, s, mx, 60) for s in (1, 2, 3) for mx in (True, False)] +
          [(67, 201, s, mx, 60) for s in (1, 2, 3) for mx in (True, False)] + [(200, 500, 1, True, 40)])
BEYOND_DEPTH = 64
# what the reference returns at 160 x 320: (seed, maximize) -> (status, nodes)
BEYOND_160 = {(2, True): (OPTIMAL, 19), (3, False): (OPTIMAL, 43), (1, True): (ITER_LIMIT, 60),
              (1, False): (ITER_LIMIT, 60), (2, False): (ITER_LIMIT, 60), (3, True): (ITER_LIMIT, 60)}

# the set above has no first child that ends LP_INFEASIBLE; this one (every structural column marked) has six among its
# 52 dives and 7 rebuilds: (m, n, seed, maximize, every, max_nodes)
BEYOND_INFEASIBLE_DIVES = (160, 320, 4, False, 1, 60)

# rebuild-heavy (max_depth 8) and dive-only (max_depth 64): boxed_mip(seed, 160, 320, True, "box", 1), 60 nodes
BOX_SEEDS = (1, 2)

TALL_SHAPE = (1100, 2300)
TALL_K = 1200
# (max_depth, max_nodes) -> (status, stats) the reference returns for tall(1), max_iter 20000
TALL_RUNS = {(64, 8): (ITER_LIMIT, (8, 119, 4368, 53, 7)), (2, 6): (ITER_LIMIT, (5, 26, 4368, 53, 2))}
TALL_MAX_ITER = 20000
TALL_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mip_bounded_large_tall.json")


def _freeze(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def problem(m, n, seed, maximize, kind, every):
    """R.boxed_mip(seed, m, n, maximize, kind, every) and its cold root: (A, b, c, lo, hi, mask, root)."""
    A, b, c, lo, hi, mask, _ = R.boxed_mip(seed, m, n, maximize, kind, every)
    root = B.bounded(A, b, c, lo, hi, maximize)
    return _freeze([A, b, c, lo, hi, mask]) + (root,)


_ref_cache = {}


def ref(key, A, b, c, lo, hi, basis, at_upper, mask, maximize, n_orig, **kw):
    """R.mip(...), computed once per key."""
    if key not in _ref_cache:
        _ref_cache[key] = R.mip(A, b, c, lo, hi, basis, at_upper, mask, maximize, n_orig, **kw)
    return _ref_cache[key]


def searched(m, n, seed, maximize, kind, every, **kw):
    """(the arguments of ctx.mip_bounded_solve_large, the reference's result) for problem(...) under the limits kw;
    None when the root is not optimal."""
    A, b, c, lo, hi, mask, root = problem(m, n, seed, maximize, kind, every)
    if root["status"] != OPTIMAL:
        return None
    args = (A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, n - m)
    key = (m, n, seed, maximize, kind, every, tuple(sorted(kw.items())))
    return args, ref(key, *args, **kw)


def host_search(resolve, A, b, c, lo, hi, basis, at_upper, mask, maximize, n_orig, eps=1e-9, int_tol=1e-6, gap=1e-9,
                max_depth=64, max_nodes=100000, max_iter=10000):
    """The search of mip_bounded_ref.c written on the host with one re-solve per node: resolve(A, b, c, lo, hi, basis,
    at_upper, maximize, n_orig, eps, max_iter) is bounded_resolve_ref.resolve or ctx.bounded_resolve_large.  A first
    child starts from its parent's final basis and flags, a second child from the recorded ones.  What a user can do
    without lp_mip_bounded_solve_large; its arithmetic is not the reference's (every node is crashed afresh), so it is
    compared by nodes and objective, never bit for bit.  Returns dict(status, found, x, obj, nodes, dives, rebuilds,
    infeasible_dives, dual, deepest)."""
    def beats(z, zs, g):
        return z > zs + g if maximize else z < zs - g

    out = dict(nodes=1, dives=0, rebuilds=0, infeasible_dives=0, dual=0, deepest=0)
    lov, hiv = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    r = resolve(A, b, c, lov, hiv, basis, at_upper, maximize, n_orig, eps, max_iter)
    out["dual"] += int(r["iters"][0])
    st, found, zstar, xs, stop, have_ab = r["status"], 0, 0.0, None, OPTIMAL, 0
    rec, L, top = [], 0, -1
    marked = np.flatnonzero(np.asarray(mask)[:n_orig])
    if st != OPTIMAL:   # the root's status, no search
        out.update(status=st, found=0, x=None, obj=float("nan"))
        return out
    while True:
        backtrack = True
        if st == OPTIMAL:
            x, z = r["x"], r["obj"]
            if not found or beats(z, zstar, gap):
                f = x[marked] - np.floor(x[marked])
                dist = np.where(f < 1.0 - f, f, 1.0 - f)
                dist = np.where(dist > int_tol, dist, 0.0)
                k = int(np.argmax(dist)) if len(marked) else 0   # the first maximum: ties to the lowest index
                jb = int(marked[k]) if len(marked) and dist[k] > 0.0 else -1
                if jb < 0:
                    found, zstar, xs = 1, z, x.copy()
                elif L == max_depth:
                    have_ab = 1
                else:
                    v = x[jb]
                    del rec[L:]
                    rec.append(dict(j=jb, v=v, down=(v - np.floor(v)) <= 0.5, taken=False, basis=r["basis"].copy(),
                                    up=r["at_upper"].copy()))
                    top = L
                    if out["nodes"] >= max_nodes:
                        stop = ITER_LIMIT
                        break
                    if rec[L]["down"]:
                        hiv[jb] = np.floor(v)
                    else:
                        lov[jb] = np.ceil(v)
                    L += 1
                    out["nodes"] += 1
                    out["dives"] += 1
                    out["deepest"] = max(out["deepest"], L)
                    r = resolve(A, b, c, lov, hiv, r["basis"], r["at_upper"], maximize, n_orig, eps, max_iter)
                    st = r["status"]
                    out["dual"] += int(r["iters"][0])
                    out["infeasible_dives"] += st == INFEASIBLE
                    backtrack = False
        elif st != INFEASIBLE:
            stop = st
            break
        if not backtrack:
            continue
        while top >= 0 and rec[top]["taken"]:
            top -= 1
        if top < 0:
            break
        rec[top]["taken"] = True
        if out["nodes"] >= max_nodes:
            stop = ITER_LIMIT
            break
        L = top + 1
        lov, hiv = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
        for R_ in rec[:L]:
            if R_["down"] != R_["taken"]:
                hiv[R_["j"]] = np.floor(R_["v"])
            else:
                lov[R_["j"]] = np.ceil(R_["v"])
        out["nodes"] += 1
        out["rebuilds"] += 1
        out["deepest"] = max(out["deepest"], L)
        r = resolve(A, b, c, lov, hiv, rec[top]["basis"], rec[top]["up"], maximize, n_orig, eps, max_iter)
        st = r["status"]
        out["dual"] += int(r["iters"][0])
    if stop != OPTIMAL:
        status = stop
    elif found:
        status = OPTIMAL   # (an abandoned node that still beats the incumbent: the callers compare found and obj only)
    else:
        status = ITER_LIMIT if have_ab else INFEASIBLE
    out.update(status=status, found=found, x=xs, obj=zstar if found else float("nan"))
    return out


def zero_mask_start(kind, rounded=None):
    """The "bound" or "cost" warm start of bounded_resolve_large_cases at 160 x 320 (seed 1, max) with the mask of
    problem(160, 320, 1, True, "mixed", 2): (A, b, c, lo, hi, basis, at_upper, mask).  "bound": the marked columns'
    bounds rounded outward, so the start can also be searched under the mask.  "cost" keeps its bounds: a rounded bound
    moves every non-basic column that sits on it, the start loses the primal feasibility the moved costs leave it as its
    only one, and the reference answers REF_BAD_ARG (rounded=True shows it); with a zero mask no bound need be an
    integer."""
    from tests import bounded_resolve_large_cases as W
    m, n = 160, 320
    A, b, c, lo, hi, basis, up = W.warm(m, n, 1, True, kind, W.cold_ref(m, n, 1, True))
    mask = problem(m, n, 1, True, "mixed", 2)[5]
    lo, hi = lo.copy(), hi.copy()
    if kind == "bound" if rounded is None else rounded:
        for j in np.flatnonzero(mask):
            lo[j] = np.floor(lo[j])
            if np.isfinite(hi[j]):
                hi[j] = np.ceil(hi[j])
    return A, b, c, lo, hi, basis, up, mask


@functools.lru_cache(maxsize=None)
def tall(seed, m=TALL_SHAPE[0], k=TALL_K, nz=3):
    """More rows and more marked columns than a block has threads: A = [A0 | I], three entries from 1..9 per column of
    A0, k integer columns in [0, 3], maximised from the slack basis (the root's primal loop starts from the identity).
    Returns (A, b, c, lo, hi, mask)."""
    rng = np.random.default_rng(seed)
    A0 = np.zeros((m, k))
    for j in range(k):
        rows = rng.choice(m, nz, replace=False)
        A0[rows, j] = rng.integers(1, 10, nz)
    b = np.floor(A0.sum(axis=1) * rng.uniform(0.8, 1.6, m)) + 0.5
    c0 = (A0.sum(axis=0) * rng.uniform(0.8, 1.2, k)).round(2)
    A = np.hstack([A0, np.eye(m)])
    c = np.r_[c0, np.zeros(m)]
    n = k + m
    lo = np.zeros(n)
    hi = np.full(n, np.inf)
    hi[:k] = 3.0
    mask = np.r_[np.ones(k, np.int32), np.zeros(m, np.int32)]
    return _freeze([A, b, c, lo, hi, mask])


def tall_args(seed=1):
    A, b, c, lo, hi, mask = tall(seed)
    m, n = A.shape
    return (A, b, c, lo, hi, np.arange(n - m, n, dtype=np.int32), np.zeros(n, np.int32), mask, True, TALL_K)


def _hex(v):
    return float(v).hex()


def pack(r):
    """A result as JSON-able data, the floats as hex strings."""
    return dict(status=int(r["status"]), found=int(r["found"]), stats=[int(v) for v in r["stats"]],
                x=[_hex(v) for v in r["x"]], obj=_hex(r["obj"]), bound=_hex(r["bound"]))


def unpack(d):
    return dict(status=d["status"], found=d["found"], stats=tuple(d["stats"]),
                x=np.array([float.fromhex(v) for v in d["x"]]), obj=float.fromhex(d["obj"]),
                bound=float.fromhex(d["bound"]))


def tall_fixture():
    """The reference's recorded results for tall_args(1): {(max_depth, max_nodes): result}."""
    with open(TALL_FIXTURE) as f:
        data = json.load(f)
    return {(e["max_depth"], e["max_nodes"]): unpack(e["result"]) for e in data["runs"]}
