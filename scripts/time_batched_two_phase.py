"""Timing of the batched two-phase simplex: 4096 LPs of lpcases.min_lp(seed, 64, 128), seeds 0..4095 (canonical
64 x 192, no starting basis), one LP per workgroup, against lp_simplex_two_phase looped over the first 128 LPs.
Prints one JSON line (committed as profiles/batched_two_phase.json)."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import lpcases  # noqa: E402

batch, m, k, runs, loop_lps = 4096, 64, 128, 7, 128
cases = [lpcases.min_lp(seed, m, k) for seed in range(batch)]
A = np.stack([q[0] for q in cases]); b = np.stack([q[1] for q in cases]); c = np.stack([q[2] for q in cases])

ctx = capi.Context(0)
p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=k)
assert p.path() == 1
p.run()   # warm-up
ms = [p.run() for _ in range(runs)]
d = p.download()
it = p.phase_iters()
p.free()

# the per-LP loop: one upload, a chain of launches and host syncs, one download per LP (host clock, ends in a sync)
for q in cases[:2]:   # warm-up
    ctx.two_phase(q[0], q[1], q[2], maximize=False, n_orig=k)
t0 = time.perf_counter()
for q in cases[:loop_lps]:
    ctx.two_phase(q[0], q[1], q[2], maximize=False, n_orig=k)
loop_ms_per_lp = (time.perf_counter() - t0) * 1e3 / loop_lps
ctx.close()

med = float(np.median(ms))
print(json.dumps({
    "workload": "lpcases.min_lp(seed, 64, 128), seeds 0..%d: canonical 64 x 192, no starting basis" % (batch - 1),
    "batch": batch, "m": m, "n": m + k,
    "batched_runs": runs, "batched_ms_median": round(med, 4), "batched_ms_min": round(min(ms), 4),
    "batched_ms_max": round(max(ms), 4), "batched_us_per_lp": round(med * 1e3 / batch, 3),
    "pivots_phase1": int(it[:, 0].sum()), "pivots_driveout": int(it[:, 1].sum()), "pivots_phase2": int(it[:, 2].sum()),
    "all_optimal": bool((d["status"] == 0).all()),
    "loop_lps": loop_lps, "loop_ms_per_lp": round(loop_ms_per_lp, 4),
    "speedup_per_lp": round(loop_ms_per_lp / (med / batch), 1),
    "kernel_source_hash": bench.kernel_source_hash()}), flush=True)
