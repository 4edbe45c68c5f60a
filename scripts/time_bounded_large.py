"""The bounded-variable simplex on the HBM tableau (lp_simplex_bounded_large) against the only way to solve the same LP
without it: every finite upper bound written as a row (tests/bounded_ref.as_rows) and lp_simplex_two_phase on the
(m+k) x (n+k) problem, in the same run.
Workloads: tests/bounded_ref.boxed_lp(1, m, n, kind) for kind "box" and "mixed" at 512 x 1024 and 2048 x 4096.
Per workload: host wall clock of the whole call (upload, every launch, download; ends in a device synchronise), the
median of RUNS calls after one warm-up call of each entry, the iteration counts, both objectives and their agreement
within 1e-7 max(1, |z|), and the tableau bytes one pivot streams in each form (16 (m+1) ld against 16 (m+k+1) ld').

  python scripts/time_bounded_large.py [out.json] [--only-m=512]     the timed run; writes profiles/bounded_large.json
                                                                     (--only-m: one shape, added to an existing file)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_bounded_large.py --calls-only
                                                                     one lp_simplex_bounded_large call per workload
                                                                     (2048 x 4096: max_iter 4000), iters in calls.json
  python scripts/time_bounded_large.py --trace DIR [out.json]        adds the kernel times of that trace to out.json:
      per workload (the trace is cut at the k_build_tableau of each call) the selector + update pairs in launch order;
      a pair whose k_simplex_update did work is a pivot, a pair whose update returned at once behind a selector that
      priced is a flip (or the last selector of a phase), the rest are the no-op pairs queued behind the end of a phase.
      The count of updates that did work must equal pivots + drive-out pivots: a flip streams no tableau."""
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

WORKLOADS = [(512, 1024, "box"), (512, 1024, "mixed"), (2048, 4096, "box"), (2048, 4096, "mixed")]
RUNS = {512: 5, 2048: 1}
MAX_ITER = 1000000
TRACE_MAX_ITER = {512: MAX_ITER, 2048: 4000}   # the traced 2048 x 4096 calls stop in phase I: the trace stays small


def _name(m, n, kind):
    return f"{kind}_{m}x{n}"


def _ld(cols):
    return (cols + 1 + 7) // 8 * 8


def _timed(fn, runs):
    ms, out = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                 "runs": runs}


def calls_only(ctx, side):
    done = {}
    for m, n, kind in WORKLOADS:
        A, b, c, lo, hi, mx = R.boxed_lp(1, m, n, kind=kind)
        g = ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=TRACE_MAX_ITER[m])
        done[_name(m, n, kind)] = dict(status=int(g["status"]), iters=g["iters"], max_iter=TRACE_MAX_ITER[m])
        with open(side, "w") as f:   # (after every call: a run cut short still says what it traced)
            json.dump(done, f)


def timed(ctx, path):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res["scenario"] = ("boxed_lp(1, m, n, kind): lp_simplex_bounded_large against lp_simplex_two_phase on as_rows(...) "
                       "in the same run; host wall clock of the whole call, median of `runs` calls after a warm-up call "
                       "of each entry at 64 x 192")
    A, b, c, lo, hi, mx = R.boxed_lp(1, 64, 192, kind="mixed")   # warm-up: code objects, the context's pools
    ctx.bounded_large(A, b, c, lo, hi, mx, 128)
    A2, b2, c2, _ = R.as_rows(A, b, c, lo, hi)
    ctx.two_phase(A2, b2, c2, maximize=mx, n_orig=A2.shape[1], pivot_rule="dantzig")
    for m, n, kind in WORKLOADS:
        A, b, c, lo, hi, mx = R.boxed_lp(1, m, n, kind=kind)
        g, t = _timed(lambda: ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=MAX_ITER), RUNS[m])
        A2, b2, c2, const = R.as_rows(A, b, c, lo, hi)
        m2, n2 = A2.shape
        r, t2 = _timed(lambda: ctx.two_phase(A2, b2, c2, maximize=mx, n_orig=n2, max_iter=MAX_ITER), RUNS[m])
        e = dict(shape=f"{m}x{n}", kind=kind, boxes=int(np.isfinite(hi).sum()), status=int(g["status"]),
                 iters=g["iters"], obj=g["obj"], bounded_large=t,
                 row_form=dict(t2, shape=f"{m2}x{n2}", status=int(r["status"]), iters=r["iters"],
                               obj=r["obj"] + const),
                 tableau_bytes_per_pivot=16 * (m + 1) * _ld(n + m),
                 row_form_tableau_bytes_per_pivot=16 * (m2 + 1) * _ld(n2 + m2))
        e["bytes_ratio_rows_over_bounded"] = round(e["row_form_tableau_bytes_per_pivot"] / e["tableau_bytes_per_pivot"], 2)
        e["time_ratio_rows_over_bounded"] = round(t2["ms_median"] / t["ms_median"], 2)
        if g["status"] == 0 and r["status"] == 0:
            z = r["obj"] + const
            e["objectives_agree"] = bool(abs(g["obj"] - z) <= 1e-7 * max(1.0, abs(z)))
            assert e["objectives_agree"], (g["obj"], z)
        else:
            e["objectives_agree"] = None
            assert g["status"] == r["status"], (g["status"], r["status"])
        res[_name(m, n, kind)] = e
        print(json.dumps({_name(m, n, kind): e}), flush=True)
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
    res["kernel_source_hash"] = bench.kernel_source_hash()
    res["commit"] = os.environ.get("LP_PROFILE_COMMIT", "")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def _cut(durations):
    """The duration (us) that separates an update that returned at once from one that streamed the tableau: two
    clusters of the log durations (Lloyd's iteration from the 5th and 95th percentile), cut at the middle between
    their centres.  (The widest gap of the sorted durations is not it: a few stragglers sit far above both modes.)"""
    x = np.log(np.asarray(durations, dtype=float))
    if len(x) < 2:
        return 0.0
    lo, hi = np.percentile(x, 5), np.percentile(x, 95)
    for _ in range(50):
        near_hi = np.abs(x - hi) < np.abs(x - lo)
        if near_hi.all() or not near_hi.any():
            break
        lo, hi = x[~near_hi].mean(), x[near_hi].mean()
    return float(np.exp(0.5 * (lo + hi)))


def add_trace(trace_dir, path):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    with open(files[-1], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    side = json.load(open(os.path.join(trace_dir, "calls.json")))
    res = json.load(open(path))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "k_build_tableau" in name:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    names = [_name(*w) for w in WORKLOADS if _name(*w) in side]
    if len(calls) != len(names):
        raise SystemExit(f"{len(calls)} calls in the trace, {len(names)} in calls.json")
    for wl, ks in zip(names, calls):
        it = side[wl]["iters"]
        upd = [d for n_, d in ks if "k_simplex_update" in n_]
        cut = _cut(upd)
        worked = sum(d > cut for d in upd)
        pairs = [(ks[i][1], ks[i + 1][1]) for i in range(len(ks) - 1)
                 if "k_simplex_select_bounded" in ks[i][0] and "k_simplex_update" in ks[i + 1][0]]
        piv = [(s, u) for s, u in pairs if u > cut]
        sel_med = float(np.median([s for s, _ in piv])) if piv else 0.0
        flip = [(s, u) for s, u in pairs if u <= cut and s > 0.5 * sel_med]
        idle = [(s, u) for s, u in pairs if u <= cut and s <= 0.5 * sel_med]
        e = dict(iters=it, max_iter=side[wl]["max_iter"], update_dispatches=len(upd), update_dispatches_that_did_work=worked,
                 pivots_plus_driveout=it[0] + it[1] + it[2], update_cut_us=round(cut, 2),
                 pivot_pairs=len(piv), flip_pairs=len(flip), idle_pairs=len(idle),
                 pivot_select_us=round(float(np.mean([s for s, _ in piv])), 2) if piv else None,
                 pivot_update_us=round(float(np.mean([u for _, u in piv])), 2) if piv else None,
                 flip_select_us=round(float(np.mean([s for s, _ in flip])), 2) if flip else None,
                 flip_update_us=round(float(np.mean([u for _, u in flip])), 2) if flip else None,
                 idle_pair_us=round(float(np.mean([s + u for s, u in idle])), 2) if idle else None)
        e["flips_stream_nothing"] = worked == e["pivots_plus_driveout"]
        res.setdefault(wl, {})["kernel_trace"] = e
        print(wl, json.dumps(e), flush=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    for a in sys.argv[1:]:   # --only-m=512: that shape's workloads alone (the timed run then extends an existing file)
        if a.startswith("--only-m="):
            WORKLOADS[:] = [w for w in WORKLOADS if w[0] == int(a.split("=")[1])]
    default = os.path.join(ROOT, "profiles", "bounded_large.json")
    if "--trace" in sys.argv:
        add_trace(args[0], args[1] if len(args) > 1 else default)
    else:
        context = capi.Context(0)
        if "--calls-only" in sys.argv:
            calls_only(context, args[0] if args else "calls.json")
        else:
            timed(context, args[0] if args else default)
        context.close()
