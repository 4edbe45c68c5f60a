"""The dual pricing rule of the bounded re-solve (LP_DUAL_DANTZIG against LP_DUAL_DEVEX) on the GPU.
Workloads:
  - the README's re-solve workload: tests/bounded_ref.boxed_lp(1, m, n, kind="box") at 512 x 1024 and 2048 x 4096 (2048
    boxes at the larger), cold-solved by lp_simplex_bounded_large_ex under Devex, then three bounds of basic columns
    tightened (tests/bounded_resolve_ref.perturb, "bound": the first seed that changes three bounds and whose warm
    result is optimal).  ROUNDS alternated rounds in one session of lp_simplex_bounded_resolve_large_ex,
    lp_simplex_bounded_resolve_large_dual_ex under LP_DUAL_DANTZIG and under LP_DUAL_DEVEX and, with --parent-lib, the
    parent build's lp_simplex_bounded_resolve_large_ex: host wall clock of the whole call (upload, every launch,
    download; ends in a device synchronise) as median, min and max, the dual pivot counts and the objectives' agreement;
  - the batch: 4096 boxed LPs of 64 x 192 (boxed_lp(seed, 64, 192, kind="mixed")), cold-solved by
    lp_simplex_bounded_batched, one to three bounds tightened each; lp_simplex_bounded_resolve_batched_ex and the
    _dual_ex entry under both rules in the same alternated way, with the dual pivots summed over the batch.
Under LP_DUAL_DANTZIG the new entries launch what the _ex entries launch: `dantzig_within_spread` says whether the new
entry's median is no slower than the slowest run of the _ex entry (the parent build's, where one was given); both
sets of figures are in the JSON.

  python scripts/time_bounded_resolve_dual_rules.py [--parent-lib=PATH] [out.json]
                                      the timed run; writes profiles/bounded_resolve_dual_rules.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_bounded_resolve_dual_rules.py --calls-only DIR/calls.json
                                      one warm call per shape and dual rule, in an order calls.json records
  python scripts/time_bounded_resolve_dual_rules.py --trace DIR [out.json]
      adds to out.json, per shape and rule, the mean and median duration of the dual selector
      (k_simplex_select_dual_bounded / k_simplex_select_dual_bounded_devex) over the launches that staged a pivot, and
      of the update launches behind them."""
import csv
import ctypes as C
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import bounded_ref as R  # noqa: E402
from tests import bounded_resolve_ref as W  # noqa: E402

SHAPES = [(512, 1024), (2048, 4096)]
BATCH, BM, BN = 4096, 64, 192
ROUNDS = 5
MAX_ITER = 1000000
DANTZIG, DEVEX = capi.DUAL_DANTZIG, capi.DUAL_DEVEX


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


class Parent:
    """The _ex entries of another build of the library (the parent commit's), on a context of its own."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        for name in ("lp_context_create", "lp_context_destroy", "lp_simplex_bounded_resolve_large_ex",
                     "lp_simplex_bounded_resolve_batched_ex"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
        self.h = C.c_void_p()
        assert self.lib.lp_context_create(0, None, C.byref(self.h)) == 0

    def close(self):
        self.lib.lp_context_destroy(self.h)

    def resolve_large(self, A, b, c, lo, hi, basis, up, maximize, n_orig):
        p = capi.pack_lp(A, b, c, basis, lo, hi, up)
        x, bo, uo = np.full(n_orig, np.nan), np.zeros(p.m, np.int32), np.zeros(p.n, np.int32)
        obj, it = np.full(1, np.nan), np.zeros(3, np.int32)
        d, i = capi._d, capi._i
        st = self.lib.lp_simplex_bounded_resolve_large_ex(self.h, d(p.A), p.m, p.n, d(p.b), d(p.c), d(p.lo), d(p.hi),
                                                          i(p.basis), i(p.at_upper), int(maximize), n_orig, capi.EPS,
                                                          MAX_ITER, d(x), i(bo), i(uo), d(obj), i(it), capi.PIVOT_DANTZIG)
        return dict(status=st, obj=float(obj[0]), iters=it.tolist())

    def resolve_batched(self, A, b, c, lo, hi, basis, up, maximize, n_orig):
        p = capi.pack_lp(A, b, c, basis, lo, hi, up, batched=True)
        B = p.batch
        x, bo, uo = np.full((B, n_orig), np.nan), np.zeros((B, p.m), np.int32), np.zeros((B, p.n), np.int32)
        obj, it, st = np.full(B, np.nan), np.zeros((B, 3), np.int32), np.zeros(B, np.int32)
        d, i = capi._d, capi._i
        rc = self.lib.lp_simplex_bounded_resolve_batched_ex(self.h, B, d(p.A), p.m, p.n, d(p.b), d(p.c), d(p.lo),
                                                            d(p.hi), i(p.basis), i(p.at_upper), int(maximize), n_orig,
                                                            capi.EPS, MAX_ITER, d(x), i(bo), i(uo), d(obj), i(it), i(st),
                                                            capi.PIVOT_DANTZIG)
        assert rc == 0
        return dict(status=st, obj=obj, iters=it)


def _workload(ctx, m, n):
    """The Devex cold solve and the first perturbation that tightens three bounds with an optimal warm result."""
    A, b, c, lo, hi, mx = R.boxed_lp(1, m, n, kind="box")
    cold = ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=MAX_ITER, pivot_rule="devex")
    assert cold["status"] == 0, cold["status"]
    cold["warm_tries"] = 0
    for pseed in range(1, 80):
        _, _, lo2, hi2 = W.perturb(pseed, "bound", b, c, lo, hi, cold["basis"], cold["x"])
        changed = int((lo2 != lo).sum() + (hi2 != hi).sum())
        if changed != 3:
            continue
        cold["warm_tries"] += 1
        g = ctx.bounded_resolve_large(A, b, c, lo2, hi2, cold["basis"], cold["at_upper"], mx, n - m, max_iter=MAX_ITER)
        if g["status"] == 0:
            return (A, b, c, lo2, hi2, cold["basis"], cold["at_upper"]), mx, pseed, int(np.isfinite(hi).sum()), cold
    raise SystemExit("no perturbation of three bounds with an optimal warm result")


def _batch_workload(ctx):
    lps = [R.boxed_lp(1 + k, BM, BN, maximize=True, kind="mixed") for k in range(BATCH)]
    A, b, c, lo, hi = (np.stack([lp[i] for lp in lps]) for i in range(5))
    cold = ctx.bounded_batched(A, b, c, lo, hi, True, max_iter=MAX_ITER)
    keep = np.flatnonzero(cold["status"] == 0)
    lo2, hi2 = lo.copy(), hi.copy()
    for k in keep:
        _, _, lo2[k], hi2[k] = W.perturb(1 + int(k), "bound", b[k], c[k], lo[k], hi[k], cold["basis"][k], cold["x"][k])
    return (A, b, c, lo2, hi2, cold["basis"], cold["at_upper"]), keep


def _within(new, old):
    """The new entry's median is no slower than the slowest run of the old one in the same alternated rounds."""
    return bool(new["ms_median"] <= old["ms_max"])


def timed(ctx, parent, path):
    res = {"scenario": f"{ROUNDS} alternated rounds in one session; host wall clock of the whole call; "
                       "dual rules LP_DUAL_DANTZIG and LP_DUAL_DEVEX of the bounded re-solve",
           "parent_build": "timed in the same rounds" if parent else "not measured (no --parent-lib)"}
    A, b, c, lo, hi, mx = R.boxed_lp(1, 64, 192, kind="mixed")   # warm-up: code objects, the context's pools
    w = ctx.bounded_large(A, b, c, lo, hi, mx)
    for rule in (None, DANTZIG, DEVEX):
        ctx.bounded_resolve_large(A, b, c, lo, hi, w["basis"], w["at_upper"], mx, dual_rule=rule)
        ctx.bounded_resolve(A, b, c, lo, hi, w["basis"], w["at_upper"], mx, dual_rule=rule)
    if parent:
        parent.resolve_large(A, b, c, lo, hi, w["basis"], w["at_upper"], mx, 192)
    for m, n in SHAPES:
        start, mx, pseed, boxes, cold = _workload(ctx, m, n)
        runs = {"ex": lambda: ctx.bounded_resolve_large(*start, mx, n - m, max_iter=MAX_ITER, pivot_rule="dantzig"),
                "dual_dantzig": lambda: ctx.bounded_resolve_large(*start, mx, n - m, max_iter=MAX_ITER, dual_rule=DANTZIG),
                "dual_devex": lambda: ctx.bounded_resolve_large(*start, mx, n - m, max_iter=MAX_ITER, dual_rule=DEVEX)}
        if parent:
            runs["parent_ex"] = lambda: parent.resolve_large(*start, mx, n - m)
        ms, out = {k: [] for k in runs}, {}
        for _ in range(ROUNDS):
            for k, fn in runs.items():
                out[k], t = _clock(fn)
                ms[k].append(t)
        e = dict(shape=f"{m}x{n}", boxes=boxes, perturb_seed=pseed, bounds_changed=3, crash_pivots=m,
                 cold_devex_iters=cold["iters"])
        for k in runs:
            e[k] = dict(_stats(ms[k]), status=int(out[k]["status"]), dual_pivots=int(out[k]["iters"][0]), obj=out[k]["obj"])
        z = e["ex"]["obj"]
        e["objectives_agree"] = bool(all(e[k]["status"] == 0 and abs(e[k]["obj"] - z) <= 1e-7 * max(1.0, abs(z)) for k in runs))
        e["dantzig_equals_ex"] = bool(e["dual_dantzig"]["obj"] == z and e["dual_dantzig"]["dual_pivots"] == e["ex"]["dual_pivots"])
        e["dantzig_within_spread"] = _within(e["dual_dantzig"], e["parent_ex" if parent else "ex"])
        e["speedup_devex_vs_dantzig"] = round(e["dual_dantzig"]["ms_median"] / e["dual_devex"]["ms_median"], 3)
        res[f"boxed_{m}x{n}"] = e
        print(json.dumps({f"boxed_{m}x{n}": e}), flush=True)
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
    # the batch
    start, keep = _batch_workload(ctx)
    runs = {"ex": lambda: ctx.bounded_resolve_batched(*start, True, BN - BM, max_iter=MAX_ITER, pivot_rule="dantzig"),
            "dual_dantzig": lambda: ctx.bounded_resolve_batched(*start, True, BN - BM, max_iter=MAX_ITER, dual_rule=DANTZIG),
            "dual_devex": lambda: ctx.bounded_resolve_batched(*start, True, BN - BM, max_iter=MAX_ITER, dual_rule=DEVEX)}
    if parent:
        runs["parent_ex"] = lambda: parent.resolve_batched(*start, True, BN - BM)
    ms, out = {k: [] for k in runs}, {}
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            out[k], t = _clock(fn)
            ms[k].append(t)
    e = dict(shape=f"{BATCH} x {BM}x{BN}", cold_optimal=int(len(keep)))
    for k in runs:
        st, it = np.asarray(out[k]["status"])[keep], np.asarray(out[k]["iters"])[keep]
        e[k] = dict(_stats(ms[k]), optimal=int((st == 0).sum()), infeasible=int((st == 4).sum()),
                    dual_pivots=int(it[:, 0].sum()), primal_pivots=int(it[:, 1].sum()))
    ok = (np.asarray(out["ex"]["status"])[keep] == 0) & (np.asarray(out["dual_devex"]["status"])[keep] == 0)
    za, zb = np.asarray(out["ex"]["obj"])[keep][ok], np.asarray(out["dual_devex"]["obj"])[keep][ok]
    e["statuses_agree"] = bool(np.array_equal(np.asarray(out["ex"]["status"]), np.asarray(out["dual_devex"]["status"])))
    e["objectives_agree"] = bool(np.all(np.abs(za - zb) <= 1e-7 * np.maximum(1.0, np.abs(za))))
    e["dantzig_equals_ex"] = bool(np.array_equal(np.asarray(out["ex"]["iters"]), np.asarray(out["dual_dantzig"]["iters"]))
                                  and np.array_equal(np.asarray(out["ex"]["obj"])[keep][ok],
                                                     np.asarray(out["dual_dantzig"]["obj"])[keep][ok]))
    e["dantzig_within_spread"] = _within(e["dual_dantzig"], e["parent_ex" if parent else "ex"])
    e["speedup_devex_vs_dantzig"] = round(e["dual_dantzig"]["ms_median"] / e["dual_devex"]["ms_median"], 3)
    res["batch"] = e
    print(json.dumps({"batch": e}), flush=True)
    res["kernel_source_hash"] = bench.kernel_source_hash()
    res["commit"] = os.environ.get("LP_PROFILE_COMMIT", "")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def calls_only(ctx, side):
    order = []

    def note(label, **kw):
        order.append(dict(label=label, **kw))
        with open(side, "w") as f:   # (after every call: a run cut short still says what it traced)
            json.dump(order, f)

    for m, n in SHAPES:
        start, mx, _, _, cold = _workload(ctx, m, n)
        note(f"setup_{m}x{n}", uploads=1 + cold["warm_tries"])   # the cold call and one warm call per perturbation tried
        for name, rule in (("dantzig", DANTZIG), ("devex", DEVEX)):
            g = ctx.bounded_resolve_large(*start, mx, n - m, max_iter=MAX_ITER, dual_rule=rule)
            note(f"{name}_{m}x{n}", uploads=1, iters=g["iters"], status=int(g["status"]))


def add_trace(trace_dir, path):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    with open(files[-1], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    order = json.load(open(os.path.join(trace_dir, "calls.json")))
    res = json.load(open(path)) if os.path.exists(path) else {}
    calls, cur = [], None
    for r in rows:   # the trace is cut at the k_build_tableau of each call
        name = r["Kernel_Name"]
        if "k_build_tableau" in name:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    if sum(entry["uploads"] for entry in order) != len(calls):
        raise SystemExit(f"{len(calls)} calls in the trace, {sum(entry['uploads'] for entry in order)} in calls.json")
    pos = 0
    for entry in order:
        pos += entry["uploads"]
        if not entry["label"].startswith("setup_"):
            entry["kernels"] = calls[pos - 1]
    for entry in order:
        if "kernels" not in entry:
            continue
        name, shape = entry["label"].split("_", 1)
        ks, live = entry["kernels"], sum(entry["iters"])
        sel, upd, seen = [], [], 0
        for k, (q, d) in enumerate(ks):
            if "k_simplex_select_dual_bounded" in q:
                seen += 1
                if seen <= live:
                    sel.append(d)
                    if k + 1 < len(ks) and "k_simplex_update" in ks[k + 1][0]:
                        upd.append(ks[k + 1][1])
        kern = sorted({re.search(r"k_simplex_select_dual_bounded\w*", q).group(0) for q, _ in ks
                       if "k_simplex_select_dual_bounded" in q})
        res.setdefault(f"boxed_{shape}", {}).setdefault("selector_kernel_trace", {})[name] = dict(
            kernel=kern, iters=entry["iters"], status=entry["status"], pivots_in_trace=len(sel),
            select_us_mean=round(float(np.mean(sel)), 2) if sel else None,
            select_us_median=round(float(np.median(sel)), 2) if sel else None,
            update_us_mean=round(float(np.mean(upd)), 2) if upd else None)
        print(shape, name, json.dumps(res[f"boxed_{shape}"]["selector_kernel_trace"][name]), flush=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    plib = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parent-lib=")]
    default = os.path.join(ROOT, "profiles", "bounded_resolve_dual_rules.json")
    if "--trace" in sys.argv:
        add_trace(args[0], args[1] if len(args) > 1 else default)
    else:
        context = capi.Context(0)
        if "--calls-only" in sys.argv:
            calls_only(context, args[0] if args else "calls.json")
        else:
            par = Parent(plib[0]) if plib else None
            timed(context, par, args[0] if args else default)
            if par:
                par.close()
        context.close()
