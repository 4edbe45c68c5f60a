"""Time of the parametric right-hand-side and cost paths of bounded-variable LPs (lp_basis_bounded_parametric_batched,
lp_basis_bounded_parametric_cost_batched) next to the only other way to the same curves: lp_simplex_bounded_resolve_batched
called once per breakpoint t of the path.
Workload: 4096 LPs of 32 x 96, tests/bounded_ref.boxed_lp(seed, 32, 96, kind="box"), seeds 0..4095, maximise (the
workload of profiles/bounded.json), cold-solved by lp_simplex_bounded_batched; the paths start at the bases and flags it
stopped at, under its statuses, along seeded directions d = u |b| and g = u (|c| + 0.25), u uniform in [-1, 1], up to
t_max = inf with max_breaks = 64.
Reports the median, min and max of 7 timed calls after one warm-up, host wall clock around the whole call (upload,
kernel, download).  `copies_and_launch` is the same call with every run status LP_INFEASIBLE, so that every workgroup
leaves at once (upload + an empty launch + download); `kernel_by_difference` is the whole call minus that.  The
comparator walks the breakpoints the path found: call k re-solves every LP at its k-th breakpoint (its last one for an
LP with fewer) from the basis and flags of call k - 1, max(nseg) calls in all; it gets the breakpoints for nothing and
still returns only values, no slopes.  Its time is the median of 3 sweeps.
Checks the first 64 LPs of both paths against tests/ref/bounded_parametric_ref.c bit for bit, and the comparator's
objectives against the paths' obj at the finite breakpoints.
Writes profiles/bounded_parametric.json (or the path given as the first argument) and prints it.
With --calls-only it makes three calls of each entry and writes nothing: the workload for
`rocprofv3 --kernel-trace --stats -- python scripts/time_bounded_parametric.py --calls-only`, which gives the kernels'
own durations."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import bounded_parametric_ref as R  # noqa: E402
from tests import bounded_ref as B  # noqa: E402

BATCH, REF_CHECKED, M, N, MAX_BREAKS = 4096, 64, 32, 96, 64


def _timed(fn, reps=7):
    fn()   # warm-up
    ms, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def _sweep(ctx, path, at, direction, got):
    """The comparator: one lp_simplex_bounded_resolve_batched call per breakpoint index.  Returns (calls, the largest
    relative difference between its objectives and the path's obj at the finite breakpoints of optimal re-solves)."""
    A, b, c, lo, hi, basis, up = at
    nseg, t = got["nseg"], got["t"]
    calls = int(nseg.max())
    worst = 0.0
    for k in range(1, calls + 1):
        kk = np.minimum(k, nseg)
        tk = t[np.arange(len(nseg)), kk]
        last = np.maximum(kk - 1, 0)
        tk = np.where(np.isfinite(tk), tk, t[np.arange(len(nseg)), last])   # an end at +inf: the breakpoint before it
        tk = np.where(nseg > 0, tk, 0.0)[:, None]
        bk, ck = (b + tk * direction, c) if path == "rhs" else (b, c + tk * direction)
        warm = ctx.bounded_resolve_batched(A, bk, ck, lo, hi, basis, up, True)
        ok = (warm["status"] == 0) & (nseg >= k) & np.isfinite(t[np.arange(len(nseg)), kk])
        if ok.any():
            want = got["obj"][np.arange(len(nseg)), kk][ok]
            worst = max(worst, float(np.max(np.abs(warm["obj"][ok] - want) / np.maximum(1.0, np.abs(want)))))
        good = warm["status"] == 0
        basis = np.where(good[:, None], warm["basis"], basis)
        up = np.where(good[:, None], warm["at_upper"], up)
    return calls, worst


def main(path, calls_only=False):
    ctx = capi.Context(0)
    lps = [B.boxed_lp(k, M, N, maximize=True, kind="box") for k in range(BATCH)]
    A, b, c, lo, hi = (np.stack([lp[i] for lp in lps]) for i in range(5))
    rng = np.random.default_rng(104729)
    d = rng.uniform(-1.0, 1.0, (BATCH, M)) * np.abs(b)
    g = rng.uniform(-1.0, 1.0, (BATCH, N)) * (np.abs(c) + 0.25)
    cold = ctx.bounded_batched(A, b, c, lo, hi, True)
    run = cold["status"]
    basis = np.where((run == 0)[:, None], cold["basis"], 0).astype(np.int32)
    at = (A, b, c, lo, hi, basis, cold["at_upper"])
    calls = {"rhs": lambda rs=run: ctx.bounded_parametric_batched(*at, d, np.inf, True, max_breaks=MAX_BREAKS,
                                                                  run_status=rs),
             "cost": lambda rs=run: ctx.bounded_parametric_cost_batched(*at, g, np.inf, True, max_breaks=MAX_BREAKS,
                                                                        run_status=rs)}
    if calls_only:
        for _ in range(3):
            calls["rhs"]()
            calls["cost"]()
        ctx.close()
        return
    none_run = np.full(BATCH, 4, np.int32)
    res = dict(
        scenario=f"{BATCH} x boxed_lp(seed, {M}, {N}, kind='box'), maximise, cold-solved by lp_simplex_bounded_batched; "
                 "paths from the bases and flags it stopped at, t_max = inf, max_breaks = 64; host wall clock of the "
                 "whole call, median of 7 after a warm-up; comparator: one lp_simplex_bounded_resolve_batched call per "
                 "breakpoint index, chained, median of 3 sweeps",
        shape=f"{M}x{N}", lps=BATCH, run_optimal=int((run == 0).sum()), max_breaks=MAX_BREAKS)
    for name, direction in (("rhs", d), ("cost", g)):
        got, tw = _timed(calls[name])
        _, t0 = _timed(lambda: calls[name](none_run))
        sel = slice(0, REF_CHECKED)
        want = R.parametric_batched(name, *(v[sel] for v in at), direction[sel], np.inf, True, max_breaks=MAX_BREAKS,
                                    run_status=run[sel])
        R.same_bits({k: v[sel] for k, v in got.items()}, want)
        (ncalls, worst), ts = _timed(lambda: _sweep(ctx, name, at, direction, got), reps=3)
        walked = int(np.maximum(got["nseg"] - 1, 0).sum())
        res[name] = dict(
            whole_call=tw, copies_and_launch=t0, kernel_by_difference_ms=round(tw["ms_median"] - t0["ms_median"], 3),
            breakpoints_walked=walked, segments=int(got["nseg"].sum()), max_nseg=int(got["nseg"].max()),
            us_per_breakpoint_whole_call=round(1e3 * tw["ms_median"] / max(walked, 1), 4),
            statuses={str(s): int((got["status"] == s).sum()) for s in sorted(set(got["status"].tolist()))},
            resolve_sweep=ts, resolve_calls=ncalls, resolve_worst_relative_difference=worst,
            sweep_over_whole_call=round(ts["ms_median"] / tw["ms_median"], 2), ref_checked=REF_CHECKED)
    ctx.close()
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--calls-only"]
    main(args[0] if args else os.path.join(ROOT, "profiles", "bounded_parametric.json"), "--calls-only" in sys.argv)
