"""Devex pricing (LP_PIVOT_DEVEX) against Dantzig's rule, in pivots and in time, on one MI355X.  Every comparison
is Devex against Dantzig in the same process on the same inputs; the Dantzig side is what the library does by default
(AUTO for a single LP, the register form for a plain batch) plus the like-for-like form (LAUNCH, the LDS form), so
that the per-pivot overhead of the weights is visible next to the difference in pivot counts.  After a warm-up run,
the median of 7 runs, variants alternating; `call_ms` is the host clock around the whole call (it ends in a device
synchronise), `solve_ms` / `kernel_ms` the HIP-event time the library reports for the launches alone.
  - single LP (seed 0), capi.gen_lp as is and column-scaled (tests/devex_ref.py: scaled_lp), at 512 x 1024,
    1024 x 2048 and 2048 x 4096: pivots, us per pivot, solve ms.  max_iter is 200000 here: Dantzig's rule passes the
    default 10000 on the scaled LPs;
  - 4096 LPs of 128 x 256 (seeds 0..4095), as is and column-scaled: total pivots and ms per form, one child process
    per form (the LDS form under Dantzig's rule is its diagnostic LP_BATCHED_STAMPS instantiation, the only way to
    select it: a few clock reads more per pivot);
  - batched two-phase, 4096 x min_lp(seed, 64, 128), as is and column-scaled: pivots per phase and ms.
`--selector-leg` runs 400 pivots of each rule on LAUNCH at 2048 x 4096 (column-scaled) and nothing else: the run to
put under rocprofv3 --kernel-trace --stats for the selectors' own kernel times.
Writes profiles/devex.json (or the path given as the first argument) and prints it."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import devex_ref as R  # noqa: E402
from tests import lpcases  # noqa: E402

RUNS = 7
SINGLE_MAX_ITER = 200000


def _lp(gen, seed, m, n):
    return capi.gen_lp(seed, m, n) if gen == "plain" else R.scaled_lp(seed, m, n)


def single(ctx, m, n, gen):
    A, b, c, basis = _lp(gen, 0, m, n)
    variants = (("devex_auto", "devex", capi.SIMPLEX_AUTO), ("dantzig_auto", "dantzig", capi.SIMPLEX_AUTO),
                ("dantzig_launch", "dantzig", capi.SIMPLEX_LAUNCH))
    probs, rec = {}, {}
    for name, rule, _ in variants:
        probs[name] = ctx.simplex_problem(A, b, c, basis, True, n - m)
        probs[name].set_pivot_rule(rule)
        rec[name] = {"call": [], "solve": []}
    for rep in range(RUNS + 1):   # (the first round is the warm-up)
        for name, _, algo in variants:
            p = probs[name]
            p.reset()
            t0 = time.perf_counter()
            rc, st = p.run(max_iter=SINGLE_MAX_ITER, algo=algo)
            call = (time.perf_counter() - t0) * 1e3
            if rep:
                rec[name]["call"].append(call)
                rec[name]["solve"].append(st.solve_ms)
            rec[name].update(status=rc, pivots=st.pivots, algo_used=st.algo_used)
    out = {}
    for name, _, _ in variants:
        q = rec[name]
        q["obj"] = probs[name].download()["obj"]
        probs[name].free()
        solve = float(np.median(q["solve"]))
        out[name] = {"status": q["status"], "pivots": q["pivots"], "algo_used": q["algo_used"],
                     "solve_ms": round(solve, 4), "call_ms": round(float(np.median(q["call"])), 4),
                     "us_per_pivot": round(solve * 1e3 / max(q["pivots"], 1), 3), "obj": q["obj"]}
    out["devex_over_dantzig_auto_solve_ms"] = round(out["devex_auto"]["solve_ms"] / out["dantzig_auto"]["solve_ms"], 3)
    out["devex_over_dantzig_pivots"] = round(out["devex_auto"]["pivots"] / out["dantzig_auto"]["pivots"], 3)
    return out


def _timed_batched(p):
    p.run()   # warm-up
    call, kern = [], []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        ms = p.run()
        call.append((time.perf_counter() - t0) * 1e3)
        kern.append(ms)
    return round(float(np.median(kern)), 4), round(float(np.median(call)), 4)


def batched_leg(form):
    """One form per child process: LP_BATCHED_STAMPS is read once per handle."""
    batch, m, n = 4096, 128, 256
    ctx = capi.Context(0)
    out = {}
    for gen in ("plain", "scaled"):
        cases = [_lp(gen, seed, m, n) for seed in range(batch)]
        A, b, c, basis = (np.stack([q[i] for q in cases]) for i in range(4))
        del cases
        p = ctx.batched_problem(A, b, c, basis, True, m)
        p.set_pivot_rule("devex" if form == "devex_lds" else "dantzig")
        kern, call = _timed_batched(p)
        d = p.download()
        p.free()
        out[gen] = {"kernel_ms": kern, "call_ms": call, "total_pivots": int(d["iters"].sum()),
                    "all_optimal": bool((d["status"] == 0).all()), "obj_sum": float(np.nansum(d["obj"]))}
    ctx.close()
    return out


def two_phase(ctx):
    batch, m, k = 4096, 64, 128
    out = {}
    for gen in ("plain", "scaled"):
        cases = [(lpcases.min_lp if gen == "plain" else R.scaled_min_lp)(seed, m, k) for seed in range(batch)]
        A, b, c = (np.stack([q[i] for q in cases]) for i in range(3))
        out[gen] = {}
        for rule in ("dantzig", "devex"):
            p = ctx.batched_two_phase_problem(A, b, c, maximize=False, n_orig=k)
            p.set_pivot_rule(rule)
            kern, call = _timed_batched(p)
            it = p.phase_iters()
            d = p.download()
            p.free()
            out[gen][rule] = {"kernel_ms": kern, "call_ms": call, "pivots_phase1": int(it[:, 0].sum()),
                              "pivots_driveout": int(it[:, 1].sum()), "pivots_phase2": int(it[:, 2].sum()),
                              "all_optimal": bool((d["status"] == 0).all()), "obj_sum": float(np.nansum(d["obj"]))}
    return out


def selector_leg():
    m, n = 2048, 4096
    A, b, c, basis = R.scaled_lp(0, m, n)
    ctx = capi.Context(0)
    for rule in ("dantzig", "devex"):
        p = ctx.simplex_problem(A, b, c, basis, True, n - m)
        p.set_pivot_rule(rule)
        for _ in range(2):
            p.reset()
            rc, st = p.run(max_iter=400, algo=capi.SIMPLEX_LAUNCH)
        print(rule, "status", rc, "pivots", st.pivots, "solve_ms", round(st.solve_ms, 3), flush=True)
        p.free()
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--batched-leg":
        print(json.dumps(batched_leg(sys.argv[2])))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--selector-leg":
        selector_leg()
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "devex.json")
    ctx = capi.Context(0)
    res = {"runs": RUNS, "single_seed0": {}}
    for m, n in ((512, 1024), (1024, 2048), (2048, 4096)):
        for gen in ("plain", "scaled"):
            res["single_seed0"][f"{m}x{n}_{gen}"] = single(ctx, m, n, gen)
            print(f"{m}x{n}_{gen}", json.dumps(res["single_seed0"][f"{m}x{n}_{gen}"]), file=sys.stderr, flush=True)
    res["batched_two_phase_4096_min_lp_64x128"] = two_phase(ctx)
    ctx.close()
    res["batched_4096x128x256"] = {}
    for form in ("dantzig_register", "dantzig_lds", "devex_lds"):
        env = dict(os.environ)
        env.pop("LP_BATCHED_STAMPS", None)
        if form == "dantzig_lds":
            env["LP_BATCHED_STAMPS"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--batched-leg", form], env=env,
                           capture_output=True, text=True, timeout=900, check=True)
        res["batched_4096x128x256"][form] = json.loads(r.stdout.strip().splitlines()[-1])
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
