"""Time of RHS and cost ranging at the final bases (lp_batched_ranging) next to the solves that produced them, and of
the single-LP call (lp_basis_ranging) on both sides of lp_basis_ranging_fits.
  - 4096 LPs tests/lpcases.min_lp(seed, 64, 128) (64 x 192): batched two-phase solve, then lp_batched_ranging;
  - 4096 LPs gen_lp(seed, 128, 256): plain batched solve from the slack bases, then lp_batched_ranging;
  - one LP gen_lp(0, 512, 1024) and one gen_lp(0, 2048, 4096) at their optimal bases: lp_basis_ranging.
Each figure is the median (and spread) of 7 timed calls after one warm-up, host wall clock around the call
(the ranging calls include their device buffers and the copies of the ends and indices back to the host).
Writes profiles/ranging.json (or the path given as the first argument) and prints it."""
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


def contains(g, b, c):
    """Every current b_i and c_j lies in its own range (the bases are optimal)."""
    ok = g["status"] == capi.OPTIMAL
    return bool(((g["b_lo"] <= b + 1e-9) & (b <= g["b_hi"] + 1e-9))[ok].all() and
                ((g["c_lo"] <= c + 1e-9) & (c <= g["c_hi"] + 1e-9))[ok].all())


def batch_case(p, b, c):
    ms = [p.run() for _ in range(8)][1:]   # the kernel's own event time, warm-up dropped
    solve = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    s = p.download()
    g = p.ranging()
    ranging = timed(p.ranging)
    return {"path": p.path(), "solve": solve, "ranging": ranging,
            "all_optimal": bool((s["status"] == capi.OPTIMAL).all()), "values_in_their_ranges": contains(g, b, c)}


def main(path):
    ctx = capi.Context(0)
    res = {}
    cases = [lpcases.min_lp(seed, 64, 128) for seed in range(4096)]
    A = np.stack([k[0] for k in cases]); b = np.stack([k[1] for k in cases]); c = np.stack([k[2] for k in cases])
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=192)
    res["two_phase_4096x64x192"] = batch_case(p, b, c)
    p.free()
    cases = [capi.gen_lp(seed, 128, 256) for seed in range(4096)]
    A = np.stack([k[0] for k in cases]); b = np.stack([k[1] for k in cases]); c = np.stack([k[2] for k in cases])
    B = np.stack([k[3] for k in cases])
    p = ctx.batched_problem(A, b, c, B, True, 128)
    res["plain_4096x128x256"] = batch_case(p, b, c)
    p.free()
    for m, n in ((512, 1024), (2048, 4096)):
        A, b, c, basis = capi.gen_lp(0, m, n)
        q = ctx.simplex_problem(A, b, c, basis, True, n - m)
        rc, st = q.run()
        assert rc == capi.OPTIMAL
        d = q.download()
        q.free()
        g = ctx.basis_ranging(A, b, c, d["basis"])
        res[f"single_{m}x{n}"] = {"fits": ctx.basis_ranging_fits(m, n), "solve_ms": round(float(st.solve_ms), 4),
                                  "ranging": timed(lambda: ctx.basis_ranging(A, b, c, d["basis"])),
                                  "status": int(g["status"]), "values_in_their_ranges": contains(g, b, c)}
    ctx.close()
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ranging.json"))
