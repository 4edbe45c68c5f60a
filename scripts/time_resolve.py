"""Warm re-solve from the old optimal bases against a cold two-phase solve, after the right-hand side changed.
Scenario: 4096 LPs gen_lp(seed, 64, 192), seeds 0..4095 (tests/resolve_ref.py: scenario):
  1. cold-solve them from the slack bases (lp_simplex_solve_batched) for the optimal bases;
  2. scale 1-4 seeded rows of b per LP by a seeded factor in [0.3, 0.9];
  3. re-solve the perturbed LPs from the old bases (lp_batched_resolve_upload + lp_batched_run: the crash of m = 64
     forced pivots per LP, then the dual or the primal simplex) and solve them cold with the batched two-phase flow
     (lp_batched_two_phase_upload + lp_batched_run): median and spread of 7 timed runs each after one warm-up, and
     the pivots of each.
Writes profiles/resolve.json (or the path given as the first argument) and prints it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import resolve_ref  # noqa: E402

BATCH, M, N = 4096, 64, 192


def timed(p, runs=7):
    p.run()   # warm-up
    ms = [p.run() for _ in range(runs)]
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def main(path):
    A, b, b2, c, basis = resolve_ref.scenario(BATCH, M, N)
    no = N - M
    ctx = capi.Context(0)
    cold = ctx.simplex_solve_batched(A, b, c, basis, True, no)
    assert (cold["status"] == capi.OPTIMAL).all()
    B = cold["basis"]

    p = ctx.batched_resolve_problem(A, b2, c, B, True, no)
    assert p.path() == 1
    warm = timed(p)
    d = p.download()
    it = p.resolve_iters()
    p.free()
    warm.update(all_optimal=bool((d["status"] == capi.OPTIMAL).all()),
                lps_dual=int((it[:, 0] > 0).sum()), lps_primal=int((it[:, 1] > 0).sum()),
                pivots_dual=int(it[:, 0].sum()), pivots_primal=int(it[:, 1].sum()),
                pivots_crash=BATCH * M)

    q = ctx.batched_two_phase_problem(A, b2, c, maximize=True, n_orig=no)
    assert q.path() == 1
    two = timed(q)
    e = q.download()
    pit = q.phase_iters()
    q.free()
    ctx.close()
    two.update(all_optimal=bool((e["status"] == capi.OPTIMAL).all()), pivots_phase1=int(pit[:, 0].sum()),
               pivots_driveout=int(pit[:, 1].sum()), pivots_phase2=int(pit[:, 2].sum()))
    ok = (d["status"] == capi.OPTIMAL) & (e["status"] == capi.OPTIMAL)
    rel = np.abs(d["obj"][ok] - e["obj"][ok]) / np.maximum(1.0, np.abs(e["obj"][ok]))
    res = {"scenario": f"{BATCH} x gen_lp(seed, {M}, {N}), b scaled on 1-4 rows by [0.3, 0.9]",
           "warm_resolve": warm, "cold_two_phase": two,
           "speedup_median": round(two["ms_median"] / warm["ms_median"], 3),
           "max_rel_objective_difference": float(rel.max()) if rel.size else None,
           "kernel_source_hash": bench.kernel_source_hash()}
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resolve.json"))
