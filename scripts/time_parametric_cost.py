"""Time of the parametric cost path (lp_batched_parametric_cost) next to the solve that produced the bases, and of the
grid approach it replaces, plus the single-LP call beyond lp_basis_parametric_cost_fits.
  - 4096 LPs tests/lpcases.min_lp(seed, 64, 128) (64 x 192): batched two-phase solve, then
    lp_batched_parametric_cost with a seeded mixed-sign g (tests/parametric_cost_ref.direction) and t_max = inf; the
    total breakpoints it found and how the paths end;
  - the grid: lp_simplex_resolve_batched from the t = 0 bases with c replaced by c + t g for every interior breakpoint
    t of the first 128 LPs' paths (one batched re-solve for all of them);
  - one LP gen_lp(0, 512, 1024) at its optimal basis: lp_basis_parametric_cost (the launch path).
Each figure is the median (and spread) of 7 timed calls after one warm-up, host wall clock around the call
(including its device buffers and the copies back to the host).
Writes profiles/parametric_cost.json (or the path given as the first argument) and prints it."""
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
from tests import parametric_cost_ref as P  # noqa: E402


def timed(fn, runs=7):
    fn()   # warm-up
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def main(path):
    ctx = capi.Context(0)
    res = {}
    batch, m, k = 4096, 64, 128
    cases = [lpcases.min_lp(seed, m, k) for seed in range(batch)]
    A = np.stack([q[0] for q in cases]); b = np.stack([q[1] for q in cases]); c = np.stack([q[2] for q in cases])
    g = np.stack([P.direction(s, c[s]) for s in range(batch)])
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=m + k)
    ms = [p.run() for _ in range(8)][1:]
    solve = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    s = p.download()
    r0 = p.parametric_cost(g)
    par = timed(lambda: p.parametric_cost(g))
    p.free()
    walked = np.isin(r0["status"], (capi.OPTIMAL, capi.UNBOUNDED, capi.ITER_LIMIT))
    breaks = int((r0["nseg"][walked] - 1).sum())
    # the grid: re-solve from the t = 0 bases with c + t g at every interior breakpoint of the first 128 paths
    G = 128
    pts = [(q, r0["t"][q, j]) for q in range(G) for j in range(1, int(r0["nseg"][q])) if walked[q]]
    cg = np.stack([c[q] + t * g[q] for q, t in pts])
    Ag, bg, Bg = A[[q for q, _ in pts]], b[[q for q, _ in pts]], s["basis"][[q for q, _ in pts]]

    def grid():
        return ctx.resolve_batched(Ag, bg, cg, Bg, False, m + k)

    r = grid()
    zg = np.asarray(r["obj"])
    zp = np.array([r0["obj"][q, j] for q in range(G) for j in range(1, int(r0["nseg"][q])) if walked[q]])
    res["two_phase_4096x64x192"] = {
        "solve": solve, "parametric_cost": par, "paths": int(walked.sum()), "breakpoints": breaks,
        "statuses": {str(int(v)): int((r0["status"] == v).sum()) for v in np.unique(r0["status"])},
        "grid_first_128": {"points": len(pts), "resolve_batched": timed(grid),
                           "grid_statuses": {str(int(v)): int((np.asarray(r["status"]) == v).sum())
                                             for v in np.unique(r["status"])},
                           "max_rel_diff_to_path": float(np.max(np.abs(zg - zp) / np.maximum(1.0, np.abs(zp))))},
    }
    A1, b1, c1, basis1 = capi.gen_lp(0, 512, 1024)
    q = ctx.simplex_problem(A1, b1, c1, basis1, True, 512)
    rc, st = q.run()
    assert rc == capi.OPTIMAL
    dl = q.download()
    q.free()
    g1 = P.direction(0, c1)
    h = ctx.basis_parametric_cost(A1, b1, c1, dl["basis"], g1)
    res["single_512x1024"] = {"fits": ctx.basis_parametric_cost_fits(512, 1024), "solve_ms": round(float(st.solve_ms), 4),
                              "parametric_cost": timed(lambda: ctx.basis_parametric_cost(A1, b1, c1, dl["basis"], g1)),
                              "status": int(h["status"]), "breakpoints": int(len(h["slope"]) - 1)}
    ctx.close()
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "parametric_cost.json"))
