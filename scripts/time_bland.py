"""Cost of Bland's pivot rule (LP_PIVOT_BLAND) against Dantzig's, in pivots and in time:
  - single LP, BASELINE configs[1] (512 x 1024, seed 0): Bland on LAUNCH, Dantzig on LAUNCH, Dantzig on AUTO
    (HIP-event solve time per pivot, best of 5 runs);
  - 4096 LPs of 128 x 256 (seeds 0..4095): Dantzig on the register form (what lp_batched_launch picks), Dantzig on
    the LDS form (its diagnostic STAMPS instantiation, the only way to select that form: a few clock reads more per
    pivot), Bland on the LDS form (median of 5 runs);
  - the batched two-phase shape of scripts/time_batched_two_phase.py (4096 x min_lp(seed, 64, 128)) under both rules.
Writes profiles/bland.json (or the path given as the first argument) and prints it."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import lpcases  # noqa: E402


def single(ctx):
    m, n = 512, 1024
    A, b, c, basis = lpcases.random_lp(0, m, n)
    out = {}
    for name, rule, algo in (("bland_launch", "bland", capi.SIMPLEX_LAUNCH),
                             ("dantzig_launch", "dantzig", capi.SIMPLEX_LAUNCH),
                             ("dantzig_auto", "dantzig", capi.SIMPLEX_AUTO)):
        p = ctx.simplex_problem(A, b, c, basis, True, n - m)
        p.set_pivot_rule(rule)
        best, piv, used = None, 0, 0
        for _ in range(6):   # (the first run is a warm-up)
            p.reset()
            rc, st = p.run(algo=algo)
            assert rc == capi.OPTIMAL
            ms, piv, used = st.solve_ms, st.pivots, st.algo_used
            best = ms if best is None else min(best, ms)
        p.free()
        out[name] = {"pivots": piv, "algo_used": used, "solve_ms": round(best, 4),
                     "us_per_pivot": round(best * 1e3 / piv, 3)}
    return out


def batched_leg(form):
    """One form per child process: LP_BATCHED_STAMPS is read once per handle."""
    batch, m, n = 4096, 128, 256
    cases = [lpcases.random_lp(seed, m, n) for seed in range(batch)]
    A, b, c, basis = (np.stack([q[i] for q in cases]) for i in range(4))
    ctx = capi.Context(0)
    p = ctx.batched_problem(A, b, c, basis, True, m)
    p.set_pivot_rule("bland" if form == "bland_lds" else "dantzig")
    p.run()
    ms = [p.run() for _ in range(5)]
    d = p.download()
    p.free()
    ctx.close()
    return {"ms_median": round(float(np.median(ms)), 4), "total_pivots": int(d["iters"].sum()),
            "all_optimal": bool((d["status"] == 0).all())}


def two_phase(ctx):
    batch, m, k = 4096, 64, 128
    cases = [lpcases.min_lp(seed, m, k) for seed in range(batch)]
    A, b, c = (np.stack([q[i] for q in cases]) for i in range(3))
    out = {}
    for rule in ("dantzig", "bland"):
        p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=k)
        p.set_pivot_rule(rule)
        p.run()
        ms = [p.run() for _ in range(5)]
        it = p.phase_iters()
        st = p.download()["status"]
        p.free()
        out[rule] = {"ms_median": round(float(np.median(ms)), 4), "pivots_phase1": int(it[:, 0].sum()),
                     "pivots_driveout": int(it[:, 1].sum()), "pivots_phase2": int(it[:, 2].sum()),
                     "all_optimal": bool((st == 0).all())}
    return out


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--batched-leg":
        print(json.dumps(batched_leg(sys.argv[2])))
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bland.json")
    ctx = capi.Context(0)
    res = {"single_512x1024_seed0": single(ctx)}
    res["batched_4096x128x256"] = {}
    for form in ("dantzig_register", "dantzig_lds", "bland_lds"):
        env = dict(os.environ)
        env.pop("LP_BATCHED_STAMPS", None)
        if form == "dantzig_lds":
            env["LP_BATCHED_STAMPS"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--batched-leg", form], env=env,
                           capture_output=True, text=True, timeout=600, check=True)
        res["batched_4096x128x256"][form] = json.loads(r.stdout.strip().splitlines()[-1])
    res["batched_two_phase_4096_min_lp_64x128"] = two_phase(ctx)
    ctx.close()
    s = res["single_512x1024_seed0"]
    res["bland_pivot_overhead"] = {
        "single_512x1024": round(s["bland_launch"]["pivots"] / s["dantzig_launch"]["pivots"], 3),
        "batched_4096x128x256": round(res["batched_4096x128x256"]["bland_lds"]["total_pivots"]
                                      / res["batched_4096x128x256"]["dantzig_register"]["total_pivots"], 3)}
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
