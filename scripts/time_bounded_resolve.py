"""The bounded-variable re-solve from old bases (lp_simplex_bounded_resolve_batched) against the cold bounded solve of
the same perturbed LPs (lp_simplex_bounded_batched), which is what a caller had to run before.
Workloads, 4096 LPs each, seeds 0..4095, maximise: tests/bounded_ref.boxed_lp(seed, m, n, kind="box") of 32 x 96 and
64 x 192, cold-solved, then one to three bounds of basic columns tightened (tests/bounded_resolve_ref.perturb, "bound").
Reports the median, min and max of 7 timed calls after one warm-up (host wall clock around the whole call: upload,
kernel, download) for both, the pivot, flip and crash counts, the share of LPs that went dual, the status histograms
and the largest relative difference of the objectives, and checks the first 64 warm results against
tests/ref/bounded_resolve_ref.c bit for bit.
Writes profiles/bounded_resolve.json (or the path given as the first argument) and prints it.
With --calls-only it makes three warm and three cold calls per shape and writes nothing: the workload for
`rocprofv3 --kernel-trace --stats -- python scripts/time_bounded_resolve.py --calls-only`, which gives the two kernels'
own durations (the host wall clock is mostly the upload of A)."""
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
from tests import bounded_ref as B  # noqa: E402
from tests import bounded_resolve_ref as W  # noqa: E402

BATCH, REF_CHECKED = 4096, 64
NAMES = {0: "optimal", 1: "unbounded", 2: "iter_limit", 3: "singular", 4: "infeasible", 5: "bad_arg"}


def _timed(fn):
    fn()   # warm-up
    ms, out = [], None
    for _ in range(7):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def _hist(status):
    return dict(sorted(collections.Counter(NAMES[int(s)] for s in status).items()))


def main(path, calls_only=False):
    ctx = capi.Context(0)
    res = {"scenario": f"{BATCH} x boxed_lp(seed, m, n, kind='box'), maximise, cold-solved, then 1-3 bounds of basic "
                       "columns tightened; warm = lp_simplex_bounded_resolve_batched from the old bases and flags, cold "
                       "= lp_simplex_bounded_batched on the same perturbed LPs; host wall clock of the whole call, "
                       "median of 7 after a warm-up"}
    for m, n in ((32, 96), (64, 192)):
        cases = [B.boxed_lp(k, m, n, maximize=True, kind="box") for k in range(BATCH)]
        A, b, c, lo, hi = (np.stack([cs[i] for cs in cases]) for i in range(5))
        first = ctx.bounded_batched(A, b, c, lo, hi, True)
        keep = np.flatnonzero(first["status"] == 0)
        lo2, hi2 = lo.copy(), hi.copy()
        for k in keep:
            _, _, lo2[k], hi2[k] = W.perturb(int(k), "bound", b[k], c[k], lo[k], hi[k], first["basis"][k], first["x"][k])
        A, b, c, lo2, hi2 = A[keep], b[keep], c[keep], lo2[keep], hi2[keep]
        basis, up = first["basis"][keep], first["at_upper"][keep]
        if calls_only:
            for _ in range(3):
                ctx.bounded_resolve_batched(A, b, c, lo2, hi2, basis, up, True, n - m)
                ctx.bounded_batched(A, b, c, lo2, hi2, True, n - m)
            continue
        warm, tw = _timed(lambda: ctx.bounded_resolve_batched(A, b, c, lo2, hi2, basis, up, True, n - m))
        cold, tc = _timed(lambda: ctx.bounded_batched(A, b, c, lo2, hi2, True, n - m))
        for k in range(REF_CHECKED):
            r = W.resolve(A[k], b[k], c[k], lo2[k], hi2[k], basis[k], up[k], True, n - m)
            assert int(warm["status"][k]) == r["status"] and [int(v) for v in warm["iters"][k]] == r["iters"], k
            assert np.array_equal(warm["basis"][k], r["basis"]) and (r["status"] or warm["obj"][k] == r["obj"]), k
        ok = (warm["status"] == 0) & (cold["status"] == 0)
        rel = np.abs(warm["obj"][ok] - cold["obj"][ok]) / np.maximum(1.0, np.abs(cold["obj"][ok]))
        wi, ci = warm["iters"], cold["iters"]
        # the crash: m forced pivots per LP unless the basis is the slack identity with zero costs (not counted by the
        # kernel; every LP whose status is not singular or infeasible-by-crossed-bounds ran all m)
        slack = np.arange(n - m, n)
        crashed = int(sum(not np.array_equal(basis[k], slack) for k in range(len(keep))
                          if not np.any(hi2[k] < lo2[k])))
        res[f"boxed_{m}x{n}"] = dict(
            shape=f"{m}x{n}", lps=int(len(keep)),
            warm=dict(tw, crash_pivots=crashed * m, dual_pivots=int(wi[:, 0].sum()), primal_pivots=int(wi[:, 1].sum()),
                      flips=int(wi[:, 2].sum()), went_dual=int((wi[:, 0] > 0).sum()), status=_hist(warm["status"])),
            cold=dict(tc, pivots_phase1=int(ci[:, 0].sum()), pivots_driveout=int(ci[:, 1].sum()),
                      pivots_phase2=int(ci[:, 2].sum()), flips=int(ci[:, 3].sum()), status=_hist(cold["status"])),
            status_mismatches=int((warm["status"] != cold["status"]).sum()),
            max_rel_obj_diff=float(rel.max()) if rel.size else 0.0,
            speedup_warm_vs_cold=round(tc["ms_median"] / tw["ms_median"], 2))
    ctx.close()
    if calls_only:
        return
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--calls-only"]
    main(args[0] if args else os.path.join(ROOT, "profiles", "bounded_resolve.json"), "--calls-only" in sys.argv)
