"""Branch-and-bound over variable bounds on two batches (lp_mip_bounded_solve_batched), host wall clock of the whole
call (upload, kernel, download), median, min and max of 7 timed calls after one warm-up.
  1. time_mip.py's workload: 4096 x gen_lp(seed, 16, 40), the 24 original columns integer, slack bases, lo = 0,
     hi = inf, max_nodes 2000: the new entry at max_depth 24 and 256, each timed call alternating with
     lp_mip_solve_batched at depth 24 (the row form: the yardstick).  Per run: nodes, pivots, time, nodes per ms, the
     status histogram and the incumbents; where both searches end optimal the objectives agree within 1e-9 relative
     (asserted; the count compared is reported).
  2. a boxed workload: 4096 x boxed_lp(k, 32, 96, kind="box"), the 64 structural columns integer with hi rounded up,
     from a cold lp_simplex_bounded_batched (timed apart), max_depth 64 and 256, max_nodes 2000.
The first 32 problems of every bounded run are checked against tests/ref/mip_bounded_ref.c bit for bit.
Writes profiles/mip_bounded.json (or the path given as the first argument) and prints it."""
import collections
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import bounded_ref, mip_bounded_ref  # noqa: E402

BATCH, MAX_NODES, REF_PROBLEMS, REPEATS = 4096, 2000, 32, 7
NAMES = {0: "optimal", 1: "unbounded", 2: "iter_limit", 3: "singular", 4: "infeasible", 5: "bad_arg"}


def summary(ms, out, pivot_cols):
    st = out["stats"]
    med = float(np.median(ms))
    hist = collections.Counter(NAMES[int(s)] for s in out["status"])
    return {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "nodes": int(st[:, 0].sum()), "pivots": int(st[:, pivot_cols].sum()),
            "nodes_per_ms": round(float(st[:, 0].sum()) / med, 1), "deepest_max": int(st[:, -1].max()),
            "status": dict(sorted(hist.items())), "optimal": int((out["status"] == 0).sum()),
            "found": int(out["found"].sum()), "hit_node_limit": int((st[:, 0] == MAX_NODES).sum())}


def check_ref(A, b, c, lo, hi, basis, up, mask, no, out, kw):
    for k in range(REF_PROBLEMS):
        r = mip_bounded_ref.mip(A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, no, **kw)
        assert r["status"] == out["status"][k] and r["stats"] == tuple(int(v) for v in out["stats"][k]), k
        assert r["found"] == out["found"][k] and (not r["found"] or r["obj"] == out["obj"][k]), k


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def workload_rows(ctx):
    m, n = 16, 40
    no = n - m
    A, b, c, basis = np.empty((BATCH, m, n)), np.empty((BATCH, m)), np.empty((BATCH, n)), np.empty((BATCH, m), np.int32)
    for k in range(BATCH):
        A[k], b[k], c[k], basis[k] = capi.gen_lp(k, m, n)
    mask = np.r_[np.ones(no), np.zeros(m)].astype(np.int32)
    lo, hi, up = np.zeros((BATCH, n)), np.full((BATCH, n), np.inf), np.zeros((BATCH, n), np.int32)

    def rows():
        return ctx.mip_batched(A, b, c, basis, mask, True, no, max_depth=24, max_nodes=MAX_NODES)

    def bounds(depth):
        return ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, maximize=True, n_orig=no,
                                             max_depth=depth, max_nodes=MAX_NODES)

    res = {"scenario": f"{BATCH} x gen_lp(seed, {m}, {n}), columns 0..{no - 1} integer, slack bases, lo = 0, hi = inf, "
                       f"max_nodes {MAX_NODES}"}
    rows()
    for depth in (24, 256):
        bounds(depth)   # warm-up
        ms_b, ms_r = [], []
        for _ in range(REPEATS):
            t, ob = timed(lambda: bounds(depth))
            ms_b.append(t)
            t, orow = timed(rows)
            ms_r.append(t)
        check_ref(A, b, c, lo, hi, basis, up, mask, no, ob, dict(max_depth=depth, max_nodes=MAX_NODES))
        both = (ob["status"] == 0) & (orow["status"] == 0)
        rel = np.abs(ob["obj"][both] - orow["obj"][both]) / np.abs(orow["obj"][both])
        assert np.all(rel <= 1e-9), float(rel.max())
        res[f"bounds_depth_{depth}"] = summary(ms_b, ob, [1, 2, 3])
        res[f"rows_depth_24_alternating_with_{depth}"] = summary(ms_r, orow, [1, 2])
        res[f"objectives_compared_depth_{depth}"] = int(both.sum())
    return res


def workload_boxed(ctx):
    m, n = 32, 96
    no = n - m
    A, b, c = np.empty((BATCH, m, n)), np.empty((BATCH, m)), np.empty((BATCH, n))
    lo, hi = np.empty((BATCH, n)), np.empty((BATCH, n))
    for k in range(BATCH):
        A[k], b[k], c[k], lo[k], hi[k], _ = bounded_ref.boxed_lp(k, m, n, maximize=True, kind="box")
    hi[:, :no] = np.ceil(hi[:, :no])
    mask = np.r_[np.ones(no), np.zeros(m)].astype(np.int32)
    ms_cold = []
    ctx.bounded_batched(A, b, c, lo, hi, True, no)
    for _ in range(REPEATS):
        t, cold = timed(lambda: ctx.bounded_batched(A, b, c, lo, hi, True, no))
        ms_cold.append(t)
    assert np.all(cold["status"] == 0)
    res = {"scenario": f"{BATCH} x boxed_lp(k, {m}, {n}, kind='box'), the {no} structural columns integer, hi rounded "
                       f"up, from the cold solve's bases and flags, max_nodes {MAX_NODES}",
           "cold_solve_ms_median": round(float(np.median(ms_cold)), 3),
           "row_form": f"lp_mip_fits({m}, {n}, 64) = {int(ctx.mip_fits(m, n, 64))}"}
    for depth in (64, 256):
        kw = dict(max_depth=depth, max_nodes=MAX_NODES)

        def run():
            return ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, cold["basis"], cold["at_upper"], maximize=True,
                                                 n_orig=no, **kw)

        run()
        ms = []
        for _ in range(REPEATS):
            t, out = timed(run)
            ms.append(t)
        check_ref(A, b, c, lo, hi, cold["basis"], cold["at_upper"], mask, no, out, kw)
        res[f"bounds_depth_{depth}"] = summary(ms, out, [1, 2, 3])
    return res


def main(path):
    ctx = capi.Context(0)
    res = {"rows_workload": workload_rows(ctx), "boxed_workload": workload_boxed(ctx),
           "timing": f"host wall clock of the whole call, median / min / max of {REPEATS} after one warm-up",
           "ref_checked_per_run": REF_PROBLEMS, "kernel_source_hash": bench.kernel_source_hash()}
    ctx.close()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mip_bounded.json"))
