"""Time of the dual solution at the final bases (lp_batched_duals) next to the solves that produced them, and of
the single-LP call (lp_basis_duals) on both sides of lp_basis_duals_fits.
  - 4096 LPs tests/lpcases.min_lp(seed, 64, 128) (64 x 192): batched two-phase solve, then lp_batched_duals;
  - 4096 LPs gen_lp(seed, 128, 256): plain batched solve from the slack bases, then lp_batched_duals;
  - one LP gen_lp(0, 512, 1024) and one gen_lp(0, 2048, 4096) at their optimal bases: lp_basis_duals.
Each figure is the median (and spread) of 7 timed calls after one warm-up, host wall clock around the call
(the duals calls include their device buffers and the copies of y, d, w back to the host).
Writes profiles/duals.json (or the path given as the first argument) and prints it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import lpcases  # noqa: E402


def timed(fn, runs=7):
    fn()   # warm-up
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def batch_case(p):
    ms = [p.run() for _ in range(8)][1:]   # the kernel's own event time, warm-up dropped
    solve = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    s = p.download()
    g = p.duals()
    duals = timed(p.duals)
    ok = s["status"] == capi.OPTIMAL
    gap = np.abs(g["w"][ok] - s["obj"][ok]) / np.maximum(1.0, np.abs(s["obj"][ok]))
    return {"path": p.path(), "solve": solve, "duals": duals, "all_optimal": bool(ok.all()),
            "max_rel_duality_gap": float(gap.max())}


def main(path):
    ctx = capi.Context(0)
    res = {}
    cases = [lpcases.min_lp(seed, 64, 128) for seed in range(4096)]
    A = np.stack([k[0] for k in cases]); b = np.stack([k[1] for k in cases]); c = np.stack([k[2] for k in cases])
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=192)
    res["two_phase_4096x64x192"] = batch_case(p)
    p.free()
    cases = [capi.gen_lp(seed, 128, 256) for seed in range(4096)]
    A = np.stack([k[0] for k in cases]); b = np.stack([k[1] for k in cases]); c = np.stack([k[2] for k in cases])
    B = np.stack([k[3] for k in cases])
    p = ctx.batched_problem(A, b, c, B, True, 128)
    res["plain_4096x128x256"] = batch_case(p)
    p.free()
    for m, n in ((512, 1024), (2048, 4096)):
        A, b, c, basis = capi.gen_lp(0, m, n)
        q = ctx.simplex_problem(A, b, c, basis, True, n - m)
        rc, st = q.run()
        assert rc == capi.OPTIMAL
        d = q.download()
        q.free()
        g = ctx.basis_duals(A, b, c, d["basis"])
        res[f"single_{m}x{n}"] = {"fits": ctx.basis_duals_fits(m), "solve_ms": round(float(st.solve_ms), 4),
                                  "duals": timed(lambda: ctx.basis_duals(A, b, c, d["basis"])),
                                  "status": int(g["status"]),
                                  "rel_duality_gap": abs(g["w"] - d["obj"]) / max(1.0, abs(d["obj"]))}
    ctx.close()
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "duals.json"))
