"""The bounded-variable re-solve on the HBM tableau (lp_simplex_bounded_resolve_large) against what a caller had to run
before it existed: the cold lp_simplex_bounded_large solve of the changed LP.
Workloads: tests/bounded_ref.boxed_lp(1, m, n, kind="box") at 512 x 1024 and 2048 x 4096, cold-solved by
lp_simplex_bounded_large, then one to three bounds of basic columns tightened (tests/bounded_resolve_ref.perturb, "bound",
the first seed whose warm result is optimal).  Then ROUNDS times in one session: the warm call from the old basis and
flags, and the cold call on the changed LP.  Per workload: host wall clock of the whole call (upload, every launch,
download; ends in a device synchronise) as median, min and max, the iteration counts of both calls, and the agreement
of the two objectives within 1e-7 max(1, |z|).
The selector comparison: capi.gen_lp(1, m, n) with lo = 0, hi = inf, cold-solved, then rows of b scaled
(tests/resolve_ref.scale_rows): lp_simplex_resolve runs k_simplex_select_dual, lp_simplex_bounded_resolve_large runs
k_simplex_select_dual_bounded, and both take the same pivots (checked).  Their whole-call times are recorded here, the
kernels' own times by the trace below.

  python scripts/time_bounded_resolve_large.py [out.json]            the timed run; writes
                                                                     profiles/bounded_resolve_large.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_bounded_resolve_large.py --calls-only DIR/calls.json
                                                                     every call once, in an order calls.json records
  python scripts/time_bounded_resolve_large.py --trace DIR [out.json]
      adds the kernel times of that trace to out.json.  The trace is cut at the k_build_tableau of each call.  For the
      warm call: the tableau build, the crash (k_crash_select + its k_simplex_update launches, the verdict, the row
      permutation), the dual pivots (k_simplex_select_dual_bounded + the updates that did work), the no-op pairs queued
      behind the end, and the rest (classification, state, extraction).  What the whole call takes beyond its kernels
      is the host set-up, the copies in both directions and the launch gaps.  For the selector comparison: the mean
      duration of each dual selector over the launches whose update did work."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import bounded_ref as R  # noqa: E402
from tests import bounded_resolve_ref as W  # noqa: E402
from tests import resolve_ref  # noqa: E402

SHAPES = [(512, 1024), (2048, 4096)]
ROUNDS = 5
MAX_ITER = 1000000


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def _workload(ctx, m, n):
    """The cold solve, and the first perturbation whose warm result is optimal: (LP, changed bounds, start, cold)."""
    A, b, c, lo, hi, mx = R.boxed_lp(1, m, n, kind="box")
    cold = ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=MAX_ITER)
    assert cold["status"] == 0, cold["status"]
    for pseed in range(1, 40):
        _, _, lo2, hi2 = W.perturb(pseed, "bound", b, c, lo, hi, cold["basis"], cold["x"])
        g = ctx.bounded_resolve_large(A, b, c, lo2, hi2, cold["basis"], cold["at_upper"], mx, n - m, max_iter=MAX_ITER)
        if g["status"] == 0:
            changed = int((lo2 != lo).sum() + (hi2 != hi).sum())
            return (A, b, c, mx), (lo, hi, lo2, hi2, pseed, changed), (cold["basis"], cold["at_upper"]), cold
    raise SystemExit("no perturbation with an optimal warm result")


def _anchor(ctx, m, n):
    """gen_lp(1, m, n), lo = 0, hi = inf, rows of b scaled: (A, b', c, lo, hi, the cold optimal basis, no flags)."""
    A, b, c, slack = capi.gen_lp(1, m, n)
    cold = ctx.simplex_solve(A, b, c, slack, True, max_iter=MAX_ITER)
    assert cold["status"] == 0
    b2 = resolve_ref.scale_rows(1, b)
    return A, b2, c, np.zeros(n), np.full(n, np.inf), cold["basis"], np.zeros(n, np.int32)


def calls_only(ctx, side):
    order = []

    def note(label, **kw):
        order.append(dict(label=label, **kw))
        with open(side, "w") as f:   # (after every call: a run cut short still says what it traced)
            json.dump(order, f)

    for m, n in SHAPES:
        (A, b, c, mx), (_, _, lo2, hi2, pseed, _), (basis, up), cold = _workload(ctx, m, n)
        note(f"setup_{m}x{n}", uploads=1 + pseed)   # the cold call and one warm call per perturbation tried
        g = ctx.bounded_resolve_large(A, b, c, lo2, hi2, basis, up, mx, n - m, max_iter=MAX_ITER)
        note(f"warm_{m}x{n}", uploads=1, iters=g["iters"], status=int(g["status"]))
        A, b2, c, lo, hi, basis, up = _anchor(ctx, m, n)
        note(f"anchor_setup_{m}x{n}", uploads=1)
        t = ctx.simplex_resolve(A, b2, c, basis, True, n - m, max_iter=MAX_ITER)
        note(f"anchor_dual_{m}x{n}", uploads=1, iters=list(t["iters"]), status=int(t["status"]))
        g = ctx.bounded_resolve_large(A, b2, c, lo, hi, basis, up, True, n - m, max_iter=MAX_ITER)
        note(f"anchor_bounded_{m}x{n}", uploads=1, iters=g["iters"], status=int(g["status"]))


def timed(ctx, path):
    res = {"scenario": f"boxed_lp(1, m, n, 'box') cold-solved by lp_simplex_bounded_large, 1-3 bounds of basic columns "
                       f"tightened; {ROUNDS} rounds in one session of the warm lp_simplex_bounded_resolve_large call and "
                       "the cold lp_simplex_bounded_large call on the changed LP; host wall clock of the whole call"}
    A, b, c, lo, hi, mx = R.boxed_lp(1, 64, 192, kind="mixed")   # warm-up: code objects, the context's pools
    w = ctx.bounded_large(A, b, c, lo, hi, mx)
    ctx.bounded_resolve_large(A, b, c, lo, hi, w["basis"], w["at_upper"], mx)
    for m, n in SHAPES:
        (A, b, c, mx), (lo, hi, lo2, hi2, pseed, changed), (basis, up), first = _workload(ctx, m, n)
        tw, tc = [], []
        for _ in range(ROUNDS):
            g, ms = _clock(lambda: ctx.bounded_resolve_large(A, b, c, lo2, hi2, basis, up, mx, n - m, max_iter=MAX_ITER))
            tw.append(ms)
            r, ms = _clock(lambda: ctx.bounded_large(A, b, c, lo2, hi2, mx, n - m, max_iter=MAX_ITER))
            tc.append(ms)
        agree = bool(g["status"] == r["status"] == 0 and abs(g["obj"] - r["obj"]) <= 1e-7 * max(1.0, abs(r["obj"])))
        e = dict(status_warm=int(g["status"]), status_cold=int(r["status"]), shape=f"{m}x{n}", boxes=int(np.isfinite(hi).sum()), perturb_seed=pseed, bounds_changed=changed,
                 first_cold_iters=first["iters"],
                 warm=dict(_stats(tw), iters=g["iters"], crash_pivots=m, obj=g["obj"]),
                 cold=dict(_stats(tc), iters=r["iters"], obj=r["obj"]), objectives_agree=agree)
        e["speedup_warm_vs_cold"] = round(e["cold"]["ms_median"] / e["warm"]["ms_median"], 2)
        # the selector comparison on the same shape
        A, b2, c, lo0, hi0, basis, up = _anchor(ctx, m, n)
        td, tb = [], []
        for _ in range(ROUNDS):
            t, ms = _clock(lambda: ctx.simplex_resolve(A, b2, c, basis, True, n - m, max_iter=MAX_ITER))
            td.append(ms)
            g, ms = _clock(lambda: ctx.bounded_resolve_large(A, b2, c, lo0, hi0, basis, up, True, n - m,
                                                             max_iter=MAX_ITER))
            tb.append(ms)
        same = bool(t["status"] == g["status"] and tuple(t["iters"]) == tuple(g["iters"][:2])
                    and np.array_equal(t["basis"], g["basis"]) and (t["status"] != 0 or t["obj"] == g["obj"]))
        e["selector_comparison"] = dict(status=int(g["status"]), dual_pivots=int(g["iters"][0]),
                                        same_pivots_and_result=same, lp_simplex_resolve=_stats(td),
                                        lp_simplex_bounded_resolve_large=_stats(tb))
        res[f"boxed_{m}x{n}"] = e
        print(json.dumps({f"boxed_{m}x{n}": e}), flush=True)
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
    res["kernel_source_hash"] = bench.kernel_source_hash()
    res["commit"] = os.environ.get("LP_PROFILE_COMMIT", "")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def _split(ks, iterations):
    """One call's kernels (name, us) in launch order -> the stages' totals.  The first `iterations` selector + update
    pairs of the loop are its pivots (and flips); the pairs queued behind them found the state word set and returned."""
    out = dict(build_us=0.0, crash_us=0.0, crash_pivots=0, loop_select_us=0.0, loop_update_us=0.0, loop_pivots=0,
               idle_us=0.0, idle_pairs=0, other_us=0.0)
    sel, live = [], False
    for i, (k, d) in enumerate(ks):
        prev = ks[i - 1][0] if i else ""
        if "k_build_tableau" in k:
            out["build_us"] += d
        elif "k_crash" in k or "k_permute_rows" in k:
            out["crash_us"] += d
            out["crash_pivots"] += "k_crash_select" in k
        elif "k_simplex_update" in k and "k_crash_select" in prev:
            out["crash_us"] += d
        elif "k_simplex_select" in k:
            live = out["loop_pivots"] < iterations
            if live:
                out["loop_select_us"] += d
                out["loop_pivots"] += 1
                sel.append(d)
            else:
                out["idle_us"] += d
                out["idle_pairs"] += 1
        elif "k_simplex_update" in k and "k_simplex_select" in prev:
            out["loop_update_us" if live else "idle_us"] += d
        else:
            out["other_us"] += d
    out = {k: (round(v, 1) if isinstance(v, float) else int(v)) for k, v in out.items()}
    out["kernels_total_us"] = round(sum(d for _, d in ks), 1)
    out["select_us_mean"] = round(float(np.mean(sel)), 2) if sel else None
    out["select_us_median"] = round(float(np.median(sel)), 2) if sel else None
    out["update_us_mean"] = round(out["loop_update_us"] / out["loop_pivots"], 2) if out["loop_pivots"] else None
    return out


def add_trace(trace_dir, path):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    with open(files[-1], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    order = json.load(open(os.path.join(trace_dir, "calls.json")))
    res = json.load(open(path))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "k_build_tableau" in name:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    if sum(entry["uploads"] for entry in order) != len(calls):
        raise SystemExit(f"{len(calls)} calls in the trace, {sum(entry['uploads'] for entry in order)} in calls.json")
    pos, picked = 0, {}
    for entry in order:
        pos += entry["uploads"]
        picked[entry["label"]] = (entry, calls[pos - 1])
    for m, n in SHAPES:
        key = f"boxed_{m}x{n}"
        if f"warm_{m}x{n}" not in picked:
            continue
        entry, ks = picked[f"warm_{m}x{n}"]
        res.setdefault(key, {})["warm_kernel_trace"] = dict(_split(ks, sum(entry["iters"])), iters=entry["iters"], status=entry["status"])
        cmp_ = {}
        for label, kern in ((f"anchor_dual_{m}x{n}", "k_simplex_select_dual"),
                            (f"anchor_bounded_{m}x{n}", "k_simplex_select_dual_bounded")):
            entry, ks = picked[label]
            s = _split(ks, sum(entry["iters"]))
            cmp_[kern] = dict(iters=entry["iters"], pivots_in_trace=s["loop_pivots"], select_us_mean=s["select_us_mean"],
                              select_us_median=s["select_us_median"], update_us_mean=s["update_us_mean"])
        res[key]["selector_kernel_trace"] = cmp_
        print(key, json.dumps(res[key]["warm_kernel_trace"]), json.dumps(cmp_), flush=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    default = os.path.join(ROOT, "profiles", "bounded_resolve_large.json")
    if "--trace" in sys.argv:
        add_trace(args[0], args[1] if len(args) > 1 else default)
    else:
        context = capi.Context(0)
        if "--calls-only" in sys.argv:
            calls_only(context, args[0] if args else "calls.json")
        else:
            timed(context, args[0] if args else default)
        context.close()
