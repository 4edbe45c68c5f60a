"""Branch-and-bound over variable bounds on the HBM tableau (lp_mip_bounded_solve_large) against what a caller had to
write before it existed: the same depth-first search on the host with one lp_simplex_bounded_resolve_large call per
node (tests/mip_bounded_large_cases.host_search: every node uploads A and crashes its basis).
Workloads: tests/mip_bounded_ref.boxed_mip(1, m, n, kind="mixed", every=2) at 512 x 1024 (200 nodes) and 2048 x 4096
(40 nodes), max_depth 64, the root from lp_simplex_bounded_large_ex under Devex.  Then ROUNDS times in one session, after
one warm-up of each: the new entry, then the host search.  Per workload: host wall clock of the whole search as median,
min and max; nodes, dual pivots and deepest level of both (the host search takes the same nodes, asserted; the
dive / rebuild split is the host search's count), crash pivots (rebuilds x m for the new entry, nodes x m for the host
search), the incumbents' agreement within 1e-9 relative (the host search is not bit-equal by construction), and once,
at 512 x 1024 only, tests/ref/mip_bounded_ref.c on one core (time, and bit-for-bit equality with the new entry).

  python scripts/time_mip_bounded_large.py [out.json]      the timed run; writes profiles/mip_bounded_large.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_mip_bounded_large.py --calls-only M
                                                           the new entry once at the shape of M rows (512 or 2048), in a
                                                           run of its own
  python scripts/time_mip_bounded_large.py --trace DIR M [out.json]
      adds the node kernel's and the staging kernels' launches and mean times from that run's kernel_stats.csv to
      out.json as kernels_M."""
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
from tests import mip_bounded_large_cases as Q  # noqa: E402
from tests import mip_bounded_ref as R  # noqa: E402

SHAPES = [(512, 1024, 200), (2048, 4096, 40)]
DEPTH = 64
ROUNDS = 5
MAX_ITER = 1000000
KERNELS = ("k_mipl_node", "k_mipl_stage_columns", "k_mipl_stage_rhs")


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def _workload(ctx, m, n):
    """The problem and its Devex root: the arguments of the search."""
    A, b, c, lo, hi, mask, mx = R.boxed_mip(1, m, n, None, "mixed", 2)
    A = np.asfortranarray(A)   # the ABI's layout: neither search pays a transpose per call
    root = ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=MAX_ITER, pivot_rule=capi.PIVOT_DEVEX)
    assert root["status"] == 0, root["status"]
    return A, b, c, lo, hi, root["basis"], root["at_upper"], mask, mx, n - m


def _resolve(ctx):
    def call(A, b, c, lo, hi, basis, up, mx, n_orig, eps, max_iter):
        return ctx.bounded_resolve_large(A, b, c, lo, hi, basis, up, mx, n_orig, eps, max_iter)
    return call


def calls_only(ctx, only_m):
    for m, n, nodes in SHAPES:
        if only_m and m != only_m:
            continue
        g = ctx.mip_bounded_solve_large(*_workload(ctx, m, n), max_depth=DEPTH, max_nodes=nodes, max_iter=MAX_ITER)
        print(m, n, g["status"], g["stats"], flush=True)


def timed(ctx, path):
    res = {"scenario": f"boxed_mip(1, m, n, 'mixed', every=2) from the Devex root of lp_simplex_bounded_large_ex, max_depth "
                       f"{DEPTH}; {ROUNDS} rounds in one session of lp_mip_bounded_solve_large and of the same search on the "
                       "host with one lp_simplex_bounded_resolve_large call per node; host wall clock of the whole search"}
    kw = dict(max_depth=DEPTH, max_iter=MAX_ITER)
    args = _workload(ctx, 64, 192)   # warm-up: code objects, the context's pools
    ctx.mip_bounded_solve_large(*args, max_nodes=10, **kw)
    Q.host_search(_resolve(ctx), *args, max_nodes=10, **kw)
    for m, n, nodes in SHAPES:
        args = _workload(ctx, m, n)
        ctx.mip_bounded_solve_large(*args, max_nodes=nodes, **kw)
        tn, tb = [], []
        for _ in range(ROUNDS):
            g, ms = _clock(lambda: ctx.mip_bounded_solve_large(*args, max_nodes=nodes, **kw))
            tn.append(ms)
            h, ms = _clock(lambda: Q.host_search(_resolve(ctx), *args, max_nodes=nodes, **kw))
            tb.append(ms)
        assert (h["nodes"], h["deepest"]) == (g["stats"][0], g["stats"][4]), (h, g["stats"])
        agree = bool(h["found"] == g["found"] and
                     (not g["found"] or abs(h["obj"] - g["obj"]) <= 1e-9 * max(1.0, abs(g["obj"]))))
        assert agree, (h["obj"], g["obj"])
        e = dict(shape=f"{m}x{n}", max_nodes=nodes, status=int(g["status"]), found=int(g["found"]), obj=g["obj"],
                 bound=g["bound"], nodes=int(g["stats"][0]), dives=h["dives"], rebuilds=h["rebuilds"],
                 infeasible_dives=int(h["infeasible_dives"]), deepest_level=int(g["stats"][4]),
                 new_entry=dict(_stats(tn), dual_pivots=int(g["stats"][1]), primal_pivots=int(g["stats"][2]),
                                flips=int(g["stats"][3]), crash_pivots=h["rebuilds"] * m),
                 host_search=dict(_stats(tb), dual_pivots=h["dual"], crash_pivots=h["nodes"] * m, status=int(h["status"]),
                                  obj=h["obj"]),
                 incumbents_agree=agree)
        e["speedup_new_vs_host_search"] = round(e["host_search"]["ms_median"] / e["new_entry"]["ms_median"], 2)
        e["crash_launch_ratio"] = round(h["rebuilds"] / h["nodes"], 3)
        if m == 512:   # the reference on one core, once
            r, ms = _clock(lambda: R.mip(*args, max_nodes=nodes, **kw))
            same = bool(r["status"] == g["status"] and r["stats"] == tuple(g["stats"]) and r["found"] == g["found"]
                        and np.array_equal(r["x"], g["x"], equal_nan=True) and (r["obj"] == g["obj"] or not g["found"])
                        and (r["bound"] == g["bound"] or (np.isnan(r["bound"]) and np.isnan(g["bound"]))))
            e["reference_one_core"] = dict(ms=round(ms, 1), bit_equal=same)
        res[f"boxed_mip_{m}x{n}"] = e
        print(json.dumps({f"boxed_mip_{m}x{n}": e}), flush=True)
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
    res["kernel_source_hash"] = bench.kernel_source_hash()
    res["commit"] = os.environ.get("LP_PROFILE_COMMIT", "")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def add_trace(trace_dir, path, label):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel stats under {trace_dir}")
    res = json.load(open(path))
    out = {}
    with open(files[-1], newline="") as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row["Name"]:
                    out[k] = dict(launches=int(row["Calls"]), us_mean=round(float(row["AverageNs"]) * 1e-3, 2),
                                  us_min=round(float(row["MinNs"]) * 1e-3, 2), us_max=round(float(row["MaxNs"]) * 1e-3, 2))
    res[label] = out
    print(json.dumps(out), flush=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    default = os.path.join(ROOT, "profiles", "mip_bounded_large.json")
    if "--trace" in sys.argv:
        add_trace(args[0], args[2] if len(args) > 2 else default, "kernels_" + args[1] if len(args) > 1 else "kernels")
    else:
        context = capi.Context(0)
        if "--calls-only" in sys.argv:
            calls_only(context, int(args[0]) if args else 0)
        else:
            timed(context, args[0] if args else default)
        context.close()
