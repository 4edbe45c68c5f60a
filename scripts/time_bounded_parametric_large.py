"""Time of the parametric right-hand-side and cost paths of a bounded-variable LP beyond one workgroup's LDS
(lp_basis_bounded_parametric_large, lp_basis_bounded_parametric_cost_large) from the optimum lp_simplex_bounded_large_ex
(LP_PIVOT_DEVEX) reaches on tests/bounded_ref.boxed_lp(1, m, n, kind="mixed") at 512 x 1024 and 2048 x 4096, along the
seeded directions of tests/bounded_parametric_ref.boxed_case (d = u |b|, g = u (|c| + 1/4), u uniform in [-1, 1] from
default_rng(104729 + 1)), with max_breaks = MAX_BREAKS.
ROUNDS alternated rounds in one session, after one warm-up round, of
  rhs, cost        the two new entries, whole calls (upload, every launch, download; ends in a device synchronise);
  resolve_rhs_*    what the parent commit offers instead: ONE lp_simplex_bounded_resolve_large call at b + t d for a t
  resolve_cost_*   inside a segment of the same path (at SAMPLES segments spread over it), or at c + t g.  A whole path
                   that way is one such call per breakpoint: the estimate is the sampled median times the breakpoints
                   walked, and it is an estimate, not a measurement of that many calls;
  duals_large      lp_basis_bounded_duals_large at the optimum: a call that is nearly all crash.  The cost path
                   crashes once; the plain cost path's way (two crashes) was not built, so "twice" is the measured call
                   plus this yardstick.
tests/ref/bounded_parametric_ref.c runs each path once on one core; the paths are compared with it bit for bit.

  python scripts/time_bounded_parametric_large.py [out.json]   the timed run; writes profiles/bounded_parametric_large.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_bounded_parametric_large.py --calls-only
      the solves and every call once per shape, nothing written: the kernels' own durations (k_bparl_select_rhs next to
      k_simplex_select_dual_bounded, k_bparl_select_cost next to k_simplex_select_bounded)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import bounded_parametric_ref as PR  # noqa: E402
from tests import bounded_ref as R  # noqa: E402

SHAPES = [(512, 1024), (2048, 4096)]
ROUNDS = 5
SAMPLES = 3
MAX_ITER = 1000000
MAX_BREAKS = 256
SEED = 1
OPTIMAL = 0


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def _inside(path, count):
    """`count` parameters t strictly inside segments spread over the path (the last one, if it runs to +inf, at one
    past its start)."""
    t, ns = path["t"], len(path["slope"])
    out = []
    for q in range(count):
        k = min(ns - 1, (q + 1) * ns // (count + 1))
        while k < ns - 1 and t[k + 1] == t[k]:
            k += 1
        hi = t[k + 1] if np.isfinite(t[k + 1]) else t[k] + 1.0
        out.append(0.5 * (t[k] + hi))
    return out


def main(path, calls_only=False):
    ctx = capi.Context(0)
    res = {"scenario": "boxed_lp(1, m, n, 'mixed') solved by lp_simplex_bounded_large_ex under LP_PIVOT_DEVEX, walked from "
                       f"the basis and flags returned along boxed_case's seeded d and g with max_breaks = {MAX_BREAKS}; "
                       f"{ROUNDS} alternated rounds in one session after a warm-up round; host wall clock of the whole "
                       "call; resolve_*: one lp_simplex_bounded_resolve_large call at a t inside a segment of the same "
                       f"path, {SAMPLES} segments per path, the path's alternative ESTIMATED as their median times the "
                       "breakpoints walked; duals_large: a call that is nearly all crash; the reference is "
                       "tests/ref/bounded_parametric_ref.c on one core, once"}
    for m, n in SHAPES:
        A, b, c, lo, hi, mx = R.boxed_lp(SEED, m, n, kind="mixed")
        opt = ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=MAX_ITER, pivot_rule="devex")
        assert opt["status"] == OPTIMAL and opt["basis"].max() < n, opt["status"]
        basis, up = opt["basis"], opt["at_upper"]
        d = np.random.default_rng(104729 + SEED).uniform(-1.0, 1.0, m) * np.abs(b)
        g = np.random.default_rng(104729 + SEED).uniform(-1.0, 1.0, n) * (np.abs(c) + 0.25)
        eps = capi.EPS
        try:   # (the crash rebuilds the optimal tableau in another order of operations: it may miss eps by rounding)
            ctx.bounded_parametric_large(A, b, c, lo, hi, basis, up, d, maximize=mx, max_breaks=0)
            ctx.bounded_parametric_cost_large(A, b, c, lo, hi, basis, up, g, maximize=mx, max_breaks=0)
        except capi.LPError:
            eps = 1e-7
        calls = dict(rhs=lambda: ctx.bounded_parametric_large(A, b, c, lo, hi, basis, up, d, maximize=mx, eps=eps,
                                                              max_breaks=MAX_BREAKS),
                     cost=lambda: ctx.bounded_parametric_cost_large(A, b, c, lo, hi, basis, up, g, maximize=mx, eps=eps,
                                                                    max_breaks=MAX_BREAKS),
                     duals_large=lambda: ctx.bounded_duals_large(A, b, c, lo, hi, basis, up))
        out = {k: fn() for k, fn in calls.items()}   # warm-up: code objects, the first allocations of this size
        print(f"{m}x{n}: solved in {opt['iters']}, rhs {len(out['rhs']['slope'])} segments (status "
              f"{out['rhs']['status']}), cost {len(out['cost']['slope'])} (status {out['cost']['status']})",
              file=sys.stderr, flush=True)
        for q, t in enumerate(_inside(out["rhs"], SAMPLES)):
            calls[f"resolve_rhs_{q}"] = lambda t=t: ctx.bounded_resolve_large(A, b + t * d, c, lo, hi, basis, up, mx,
                                                                             max_iter=MAX_ITER)
        for q, t in enumerate(_inside(out["cost"], SAMPLES)):
            calls[f"resolve_cost_{q}"] = lambda t=t: ctx.bounded_resolve_large(A, b, c + t * g, lo, hi, basis, up, mx,
                                                                              max_iter=MAX_ITER)
        for k, fn in calls.items():
            if k not in out:
                out[k] = fn()
        if calls_only:
            continue
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                out[k], t = _clock(fn)
                ms[k].append(t)
        entry = dict(shape=f"{m}x{n}", solve_iters=[int(v) for v in opt["iters"]], max_breaks=MAX_BREAKS, eps=eps,
                     duals_large=_stats(ms["duals_large"]))
        crash = float(np.median(ms["duals_large"]))
        for p, direction in (("rhs", d), ("cost", g)):
            got = out[p]
            want, ref_ms = _clock(lambda: PR.parametric(p, A, b, c, lo, hi, basis, up, direction, maximize=mx, eps=eps,
                                                        max_breaks=MAX_BREAKS))
            PR.same_bits(got, PR.trim(want))
            ns = len(got["slope"])
            breaks = ns - 1 + (got["status"] != OPTIMAL)   # breakpoints walked (the last segment's end counts if blocked)
            mine = float(np.median(ms[p]))
            samples = [k for k in calls if k.startswith(f"resolve_{p}_")]
            each = float(np.median([np.median(ms[k]) for k in samples]))
            flips = int(((got["enter"] == got["leave"]) & (got["leave"] >= 0)).sum())
            entry[p] = dict(_stats(ms[p]), status=int(got["status"]), segments=ns, breakpoints=breaks, flips=flips,
                            upper_side_leaves=int(((got["side"] == 1) & (got["enter"] != got["leave"])).sum()),
                            zero_length_segments=int((np.diff(got["t"][:ns]) == 0.0).sum()),
                            ms_beyond_the_crash_per_breakpoint=round((mine - crash) / max(breaks, 1), 4),
                            resolve_large_samples={k: dict(_stats(ms[k]), status=int(out[k]["status"]),
                                                           iters=[int(v) for v in out[k]["iters"]]) for k in samples},
                            resolve_large_per_call_ms=round(each, 3),
                            one_resolve_large_per_breakpoint_ms_estimated=round(each * breaks, 1),
                            estimated_alternative_over_this=round(each * breaks / mine, 1),
                            reference_one_core_ms=round(ref_ms, 1),
                            reference_over_this=round(ref_ms / mine, 1), equal_to_the_reference_bit_for_bit=True)
        entry["cost"]["with_a_second_crash_ms_estimated"] = round(float(np.median(ms["cost"])) + crash, 3)
        entry["cost"]["single_crash_over_the_estimate"] = round(float(np.median(ms["cost"])) /
                                                               (float(np.median(ms["cost"])) + crash), 3)
        res[f"mixed_{m}x{n}"] = entry
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
    main(args[0] if args else os.path.join(ROOT, "profiles", "bounded_parametric_large.json"),
         "--calls-only" in sys.argv)
