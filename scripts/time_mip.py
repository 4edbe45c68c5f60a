"""Depth-first branch-and-bound on a batch of integer LPs (lp_mip_solve_batched).
Workload: 4096 problems gen_lp(seed, 16, 40), seeds 0..4095: canonical 16 x 40, the 24 original columns integer, the
slack bases as root starts, max_depth 24, max_nodes MAX_NODES.  Reports the median, min and max of 7 timed calls
after one warm-up (wall clock around the call: upload, kernel, download), total nodes and pivots, the status
histogram and how many problems hit the node limit, and tests/ref/mip_ref.c on one CPU core over the first 128
problems as a per-problem speedup.  Every GPU result of the first 128 is checked against the reference.
Writes profiles/mip.json (or the path given as the first argument) and prints it."""
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
from tests import mip_ref  # noqa: E402

BATCH, M, N, DEPTH, MAX_NODES, REF_PROBLEMS = 4096, 16, 40, 24, 2000, 128
NAMES = {0: "optimal", 1: "unbounded", 2: "iter_limit", 3: "singular", 4: "infeasible", 5: "bad_arg"}


def main(path):
    A, b, c, basis = np.empty((BATCH, M, N)), np.empty((BATCH, M)), np.empty((BATCH, N)), np.empty((BATCH, M), np.int32)
    for k in range(BATCH):
        A[k], b[k], c[k], basis[k] = capi.gen_lp(k, M, N)
    no = N - M
    mask = np.r_[np.ones(no), np.zeros(M)].astype(np.int32)
    kw = dict(max_depth=DEPTH, max_nodes=MAX_NODES)
    ctx = capi.Context(0)
    ctx.mip_batched(A, b, c, basis, mask, True, no, **kw)   # warm-up
    ms = []
    for _ in range(7):
        t0 = time.perf_counter()
        out = ctx.mip_batched(A, b, c, basis, mask, True, no, **kw)
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    st = out["stats"]
    hist = collections.Counter(NAMES[int(s)] for s in out["status"])
    t0 = time.perf_counter()
    for k in range(REF_PROBLEMS):
        r = mip_ref.mip(A[k], b[k], c[k], basis[k], mask, True, no, **kw)
        assert r["status"] == out["status"][k] and r["stats"] == tuple(int(v) for v in st[k]), k
        assert np.array_equal(np.isnan(r["x"]), np.isnan(out["x"][k])) and r["found"] == out["found"][k], k
    ref_ms = (time.perf_counter() - t0) * 1e3 / REF_PROBLEMS
    gpu_ms = float(np.median(ms)) / BATCH
    res = {"scenario": f"{BATCH} x gen_lp(seed, {M}, {N}), columns 0..{no - 1} integer, slack bases, "
                       f"max_depth {DEPTH}, max_nodes {MAX_NODES}",
           "ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
           "nodes": int(st[:, 0].sum()), "pivots_dual": int(st[:, 1].sum()), "pivots_primal": int(st[:, 2].sum()),
           "deepest_max": int(st[:, 3].max()), "status": dict(sorted(hist.items())),
           "hit_node_limit": int((st[:, 0] == MAX_NODES).sum()), "found": int(out["found"].sum()),
           "ref_ms_per_problem_one_core": round(ref_ms, 4), "gpu_ms_per_problem": round(gpu_ms, 6),
           "speedup_per_problem": round(ref_ms / gpu_ms, 1), "ref_checked": REF_PROBLEMS,
           "kernel_source_hash": bench.kernel_source_hash()}
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mip.json"))
