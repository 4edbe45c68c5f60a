"""The bounded-variable simplex on the HBM tableau under each pivot rule (lp_simplex_bounded_large_ex): Dantzig's rule
through _ex against lp_simplex_bounded_large in the same run (the same kernels: any difference beyond the spread of the
rounds is a bug), Devex pricing against both, and Bland's rule under an iteration cap for completeness.
Workloads: tests/bounded_ref.boxed_lp(1, m, n, kind) for kind "box" and "mixed" at 512 x 1024 and 2048 x 4096, as they
are and column-scaled (column j of A and c_j times s_j, lo_j and hi_j divided by s_j, s_j = 10**k with k uniform in
-3 .. 3 from default_rng(1): the same LP in other units, which Dantzig's rule feels and Devex mostly does not).
Per workload and entry: host wall clock of the whole call (upload, every launch, download; ends in a device synchronise)
as the median, min and max of ROUNDS alternated rounds (plain, Dantzig through _ex, Devex, ... five times; one round on
the column-scaled 2048 x 4096 LPs, whose Dantzig solves take minutes), the iteration counts, and the agreement of the
objectives within 1e-7 max(1, |z|).  Bland's rule runs once per workload with max_iter = BLAND_MAX_ITER per phase.

  python scripts/time_bounded_large_rules.py [out.json]
      the driver: touches no GPU itself; starts one child per workload (--workload NAME), then the kernel-trace child,
      each under its own `timeout`, and stops at the first one that fails.  Writes profiles/bounded_large_rules.json.
  python scripts/time_bounded_large_rules.py --workload NAME out.json       one workload's timed rounds, added to out.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_bounded_large_rules.py --calls-only DIR/calls.json
      one call per rule on the "mixed" LP of each shape with max_iter = TRACE_MAX_ITER (the trace stays small), in an
      order calls.json records
  python scripts/time_bounded_large_rules.py --trace DIR out.json
      adds to out.json, per shape and rule, the mean duration of the selector over the launches that priced (a pivot
      or a flip; the no-op launches queued behind the end of a phase take less than half the median and are left
      out) and of the k_simplex_update launches that streamed the tableau (the it[0] + it[2] longest behind that
      selector: one per pivot).  The trace is cut at the k_build_tableau of each call."""
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 1024), (2048, 4096)]
KINDS = ("box", "mixed")
ROUNDS = 5
SCALED_ROUNDS = {512: 5, 2048: 1}
MAX_ITER = 1000000
BLAND_MAX_ITER = 20000
TRACE_MAX_ITER = 2000
STEP_TIMEOUT_S = {512: 240, 2048: 1100}
TRACE_TIMEOUT_S = 600
SELECTORS = {"dantzig": "k_simplex_select_bounded", "bland": "k_simplex_select_bounded_bland",
             "devex": "k_simplex_select_bounded_devex"}


SCENARIO = ("tests/bounded_ref.boxed_lp(1, m, n, kind), as it is and column-scaled (s_j = 10**k, k in -3..3, "
            "default_rng(1)): lp_simplex_bounded_large (plain), lp_simplex_bounded_large_ex under Dantzig's rule and Devex in "
            "alternated rounds of one session, host wall clock of the whole call; Bland once with max_iter 20000 per phase; "
            "kernel_trace_mixed from a rocprofv3 --kernel-trace run of its own (max_iter 2000)")


def _name(m, n, kind, scaled):
    return f"{kind}_{m}x{n}" + ("_scaled" if scaled else "")


WORKLOADS = {_name(m, n, kind, sc): (m, n, kind, sc) for m, n in SHAPES for sc in (False, True) for kind in KINDS}


def workload(m, n, kind, scaled):
    from tests import bounded_ref as R
    A, b, c, lo, hi, mx = R.boxed_lp(1, m, n, kind=kind)
    if scaled:
        s = 10.0 ** np.random.default_rng(1).integers(-3, 4, size=n)
        A, c, lo, hi = A * s, c * s, lo / s, hi / s
    return A, b, c, lo, hi, mx


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def timed_workload(name, path):
    import bench  # (kernel_source_hash)
    from simplexmethod_amd import capi
    from tests import bounded_ref as R
    m, n, kind, scaled = WORKLOADS[name]
    ctx = capi.Context(0)
    A, b, c, lo, hi, mx = R.boxed_lp(1, 64, 192, kind="mixed")   # warm-up: code objects, the context's pools
    ctx.bounded_large(A, b, c, lo, hi, mx, 128)
    for rule in SELECTORS:
        ctx.bounded_large(A, b, c, lo, hi, mx, 128, pivot_rule=rule)
    A, b, c, lo, hi, mx = workload(m, n, kind, scaled)
    entries = {"plain": None, "dantzig": "dantzig", "devex": "devex"}
    ms = {k: [] for k in entries}
    out = {}
    for _ in range(SCALED_ROUNDS[m] if scaled else ROUNDS):
        for key, rule in entries.items():
            t0 = time.perf_counter()
            out[key] = ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=MAX_ITER, pivot_rule=rule)
            ms[key].append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    bl = ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=BLAND_MAX_ITER, pivot_rule="bland")
    bland_ms = (time.perf_counter() - t0) * 1e3
    ctx.close()
    p, d, v = out["plain"], out["dantzig"], out["devex"]
    same = bool(p["status"] == d["status"] and p["iters"] == d["iters"] and np.array_equal(p["basis"], d["basis"])
                and np.array_equal(p["at_upper"], d["at_upper"]) and (p["status"] != 0 or p["obj"] == d["obj"]))
    assert same, "Dantzig's rule through _ex differs from the entry without a rule"
    e = dict(shape=f"{m}x{n}", kind=kind, column_scaled=scaled, boxes=int(np.isfinite(hi).sum()))
    for key in entries:
        e[key] = dict(_stats(ms[key]), status=int(out[key]["status"]), iters=out[key]["iters"],
                      obj=out[key]["obj"] if out[key]["status"] == 0 else None)
    e["bland"] = dict(ms=round(bland_ms, 3), max_iter=BLAND_MAX_ITER, status=int(bl["status"]), iters=bl["iters"])
    e["dantzig_ex_equals_plain"] = same
    e["dantzig_ex_over_plain"] = round(e["dantzig"]["ms_median"] / e["plain"]["ms_median"], 4)
    e["speedup_devex_vs_plain"] = round(e["plain"]["ms_median"] / e["devex"]["ms_median"], 2)
    if p["status"] == 0 and v["status"] == 0:
        e["objectives_agree"] = bool(abs(p["obj"] - v["obj"]) <= 1e-7 * max(1.0, abs(p["obj"])))
    else:
        e["objectives_agree"] = None
    res = json.load(open(path)) if os.path.exists(path) else {}
    res["scenario"] = SCENARIO
    res[name] = e
    res["kernel_source_hash"] = bench.kernel_source_hash()
    res["commit"] = os.environ.get("LP_PROFILE_COMMIT", "")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps({name: e}), flush=True)


def calls_only(side):
    from simplexmethod_amd import capi
    ctx = capi.Context(0)
    order = []
    for m, n in SHAPES:
        A, b, c, lo, hi, mx = workload(m, n, "mixed", False)
        for rule in SELECTORS:
            g = ctx.bounded_large(A, b, c, lo, hi, mx, n - m, max_iter=TRACE_MAX_ITER, pivot_rule=rule)
            order.append(dict(shape=f"{m}x{n}", rule=rule, status=int(g["status"]), iters=g["iters"]))
            with open(side, "w") as f:   # (after every call: a run cut short still says what it traced)
                json.dump(order, f)
    ctx.close()


def add_trace(trace_dir, path):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel trace under {trace_dir}")
    with open(files[-1], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    order = json.load(open(os.path.join(trace_dir, "calls.json")))
    res = json.load(open(path)) if os.path.exists(path) else {}
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "k_build_tableau" in name:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    if len(calls) != len(order):
        raise SystemExit(f"{len(calls)} calls in the trace, {len(order)} in calls.json")
    out = {}
    for entry, ks in zip(order, calls):
        kern = SELECTORS[entry["rule"]]
        it = entry["iters"]
        pairs = [(ks[i][1], ks[i + 1][1]) for i in range(len(ks) - 1)
                 if re.search(kern + r"(?![A-Za-z_])", ks[i][0]) and "k_simplex_update" in ks[i + 1][0]]
        sel = np.array([s for s, _ in pairs])
        worked = sel[sel > 0.5 * np.median(sel)]          # the launches that priced: pivots and flips alike
        upd = np.sort([u for _, u in pairs])[::-1][:it[0] + it[2]]   # one update streams the tableau per pivot
        out.setdefault(entry["shape"], {})[entry["rule"]] = dict(
            selector=kern, iters=it, status=entry["status"], max_iter=TRACE_MAX_ITER, pairs=len(pairs),
            selector_launches_that_priced=int(len(worked)), select_us=round(float(worked.mean()), 2),
            select_us_median=round(float(np.median(worked)), 2), pivot_updates=int(len(upd)),
            update_us=round(float(upd.mean()), 2) if len(upd) else None)
    res["kernel_trace_mixed"] = out
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(out), flush=True)


def drive(path):
    """Every GPU step as a child under its own time limit; nothing further starts after a failure."""
    me = os.path.abspath(__file__)
    if os.path.exists(path):
        os.remove(path)
    for name, (m, _, _, _) in WORKLOADS.items():
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[m]), sys.executable, me, "--workload", name, path]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            raise SystemExit(f"{name}: exit status {rc}; nothing further is started")
    trace_dir = os.path.join(os.path.dirname(os.path.abspath(path)), "bounded_large_rules_trace")
    shutil.rmtree(trace_dir, ignore_errors=True)
    os.makedirs(trace_dir)
    cmd = ["timeout", "-k", "10", str(TRACE_TIMEOUT_S), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
           "-d", trace_dir, "--", sys.executable, me, "--calls-only", os.path.join(trace_dir, "calls.json")]
    rc = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.DEVNULL).returncode
    if rc != 0:
        raise SystemExit(f"kernel trace: exit status {rc}")
    add_trace(trace_dir, path)
    shutil.rmtree(trace_dir, ignore_errors=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    default = os.path.join(ROOT, "profiles", "bounded_large_rules.json")
    if "--workload" in sys.argv:
        timed_workload(args[0], args[1] if len(args) > 1 else default)
    elif "--calls-only" in sys.argv:
        calls_only(args[0] if args else "calls.json")
    elif "--trace" in sys.argv:
        add_trace(args[0], args[1] if len(args) > 1 else default)
    else:
        drive(args[0] if args else default)
