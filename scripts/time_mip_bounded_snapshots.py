"""Branch-and-bound beyond LDS with tableau snapshots (lp_mip_bounded_solve_large_ex) against the same search without
them, on the workloads of scripts/time_mip_bounded_large.py: tests/mip_bounded_ref.boxed_mip(1, m, n, kind="mixed",
every=2) from the Devex root of lp_simplex_bounded_large_ex,
  512x1024_200      512 x 1024, max_depth 64, 200 nodes: about half the nodes are second children;
  2048x4096_dive    2048 x 4096, max_depth 64, 40 nodes: every node after the root is a first child;
  2048x4096_rebuild 2048 x 4096, max_depth 4, 32 nodes: the same problem searched breadth-limited, so that about half the
                    nodes are second children (each rebuild is 2048 crash launch pairs).
Per workload, ROUNDS times in one session after one warm-up of each, alternated: the _ex entry with 0, 4 and max_depth
snapshots.  Host wall clock of the whole call as median, min and max; nodes, second children restored and rebuilt, crash
launch pairs saved (restored x m), the bytes of the slots the search wrote, and whether the variants agree (status,
found, nodes; the objective within 1e-9 relative), and the ratios of max_depth and 4 snapshots to 0.

Against the parent commit (--ab-parent): its lp_mip_bounded_solve_large and this build's _ex entry with 0 snapshots, each
in a process of its own with the library loaded through the same raw binding on the process's only context, the
processes alternated, ROUNDS of each, one warm-up and one timed call per workload and process.  (A second build loaded
into the session above runs 2 to 6 % slower than the first whichever build it is: a copy of this build in that place is
as slow as the parent's there.  So the two are not compared in one process.)  Recorded: both medians with min and max,
bit-equality of the results, and whether the median with 0 snapshots lies inside the parent's min-max.

  python scripts/time_mip_bounded_snapshots.py [out.json]       the timed run; writes profiles/mip_bounded_snapshots.json
  python scripts/time_mip_bounded_snapshots.py --ab-parent=PARENT_LIB [out.json]
                                                      adds the comparison with the parent build to out.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_mip_bounded_snapshots.py --calls-only NAME
                                                      the entry once with max_depth snapshots on the workload NAME, in a
                                                      run of its own
  python scripts/time_mip_bounded_snapshots.py --trace DIR NAME [out.json]
      adds the save, restore and second-child kernels' launches and mean times from that run's kernel_stats.csv to
      out.json as kernels_NAME."""
import csv
import ctypes as C
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
from tests import mip_bounded_ref as R  # noqa: E402

# name -> (m, n, max_depth, max_nodes)
WORKLOADS = {"512x1024_200": (512, 1024, 64, 200), "2048x4096_dive": (2048, 4096, 64, 40),
             "2048x4096_rebuild": (2048, 4096, 4, 32)}
ROUNDS = 5
MAX_ITER = 1000000
KERNELS = ("k_mipl_save", "k_mipl_restore", "k_mipl_second_child", "k_mipl_node")


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


class Build:
    """One build of the library through a raw binding of its own: lp_mip_bounded_solve_large (snapshots None: every
    build has it) or lp_mip_bounded_solve_large_ex, on a context of its own."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        for name in ("lp_context_create", "lp_context_destroy", "lp_mip_bounded_solve_large",
                     "lp_mip_bounded_solve_large_ex"):
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = capi.SIGNATURES[name]
        self.h = C.c_void_p()
        assert self.lib.lp_context_create(0, None, C.byref(self.h)) == 0

    def close(self):
        self.lib.lp_context_destroy(self.h)

    def solve(self, A, b, c, lo, hi, basis, up, mask, maximize, n_orig, max_depth, max_nodes, snapshots=None):
        p = capi.pack_lp(A, b, c, basis, lo, hi, up)
        mask = np.ascontiguousarray(mask, dtype=np.int32)
        x, obj, bound = np.full(n_orig, np.nan), np.full(1, np.nan), np.full(1, np.nan)
        found, stats = np.zeros(1, np.int32), np.zeros(7, np.int32)
        d, i = capi._d, capi._i
        call = (self.h, d(p.A), p.m, p.n, d(p.b), d(p.c), d(p.lo), d(p.hi), i(p.basis), i(p.at_upper), int(maximize),
                n_orig, i(mask), capi.EPS, capi.INT_TOL, capi.GAP, max_depth, max_nodes, MAX_ITER, d(x), d(obj), d(bound),
                i(found), i(stats))
        if snapshots is None:
            st = self.lib.lp_mip_bounded_solve_large(*call)
        else:
            st = self.lib.lp_mip_bounded_solve_large_ex(*call, snapshots)
        return dict(status=st, found=int(found[0]), x=[float(v).hex() for v in x], obj=float(obj[0]).hex(),
                    bound=float(bound[0]).hex(), stats=[int(v) for v in stats[:5]])


_roots = {}


def _workload(ctx, m, n):
    """The problem and its Devex root: the arguments of the search (one root per shape)."""
    if (m, n) not in _roots:
        A, b, c, lo, hi, mask, mx = R.boxed_mip(1, m, n, None, "mixed", 2)
        A = np.asfortranarray(A)   # the ABI's layout: no variant pays a transpose per call
        root = ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=MAX_ITER, pivot_rule=capi.PIVOT_DEVEX)
        assert root["status"] == 0, root["status"]
        _roots[(m, n)] = (A, b, c, lo, hi, root["basis"], root["at_upper"], mask, mx, n - m)
    return _roots[(m, n)]


def calls_only(ctx, name):
    m, n, depth, nodes = WORKLOADS[name]
    g = ctx.mip_bounded_solve_large(*_workload(ctx, m, n), max_depth=depth, max_nodes=nodes, max_iter=MAX_ITER,
                                    snapshots=depth)
    print(name, g["status"], g["stats"], flush=True)


def _agree(a, b):
    return bool(a["status"] == b["status"] and a["found"] == b["found"] and a["stats"][0] == b["stats"][0] and
                (not a["found"] or abs(a["obj"] - b["obj"]) <= 1e-9 * max(1.0, abs(a["obj"]))))


def timed(ctx, path):
    res = {"scenario": "boxed_mip(1, m, n, 'mixed', every=2) from the Devex root of lp_simplex_bounded_large_ex; per workload "
                       f"{ROUNDS} alternated rounds in one session, after a warm-up of each, of lp_mip_bounded_solve_large_ex "
                       "with 0, 4 and max_depth snapshots; host wall clock of the whole call",
           "parent_build": "not measured (no --ab-parent run)"}
    small = _workload(ctx, 64, 192)   # warm-up: code objects, the context's pools
    ctx.mip_bounded_solve_large(*small, max_depth=64, max_nodes=10, max_iter=MAX_ITER, snapshots=4)
    for name, (m, n, depth, nodes) in WORKLOADS.items():
        args = _workload(ctx, m, n)
        kw = dict(max_depth=depth, max_nodes=nodes, max_iter=MAX_ITER)
        runs = {"k0": lambda: ctx.mip_bounded_solve_large(*args, snapshots=0, **kw),
                "k4": lambda: ctx.mip_bounded_solve_large(*args, snapshots=4, **kw),
                "kmax": lambda: ctx.mip_bounded_solve_large(*args, snapshots=depth, **kw)}
        ms = {k: [] for k in runs}
        out = {}
        for k, fn in runs.items():
            fn()
        for _ in range(ROUNDS):
            for k, fn in runs.items():
                out[k], t = _clock(fn)
                ms[k].append(t)
        g0 = out["k0"]
        e = dict(shape=f"{m}x{n}", max_depth=depth, max_nodes=nodes, status=int(g0["status"]), found=int(g0["found"]),
                 nodes=int(g0["stats"][0]), deepest_level=int(g0["stats"][4]), second_children=int(g0["stats"][6]),
                 slot_bytes=ctx.mip_bounded_snapshot_bytes(m, n, 1))
        for k, snapshots in (("k0", 0), ("k4", 4), ("kmax", depth)):
            g = out[k]
            slots = min(snapshots, depth, int(g["stats"][4]))   # the slots the search wrote: levels 0 .. deepest - 1
            e[k] = dict(_stats(ms[k]), snapshots=snapshots, nodes=int(g["stats"][0]), dual_pivots=int(g["stats"][1]),
                        restored=int(g["stats"][5]), rebuilt=int(g["stats"][6]),
                        crash_launch_pairs_saved=int(g["stats"][5]) * m, slots_written=slots,
                        slot_bytes_taken=ctx.mip_bounded_snapshot_bytes(m, n, slots), agrees_with_k0=_agree(g, g0))
            assert e[k]["agrees_with_k0"], (name, k, g["stats"], g0["stats"])
        e["speedup_kmax_vs_k0"] = round(e["k0"]["ms_median"] / e["kmax"]["ms_median"], 3)
        e["speedup_k4_vs_k0"] = round(e["k0"]["ms_median"] / e["k4"]["ms_median"], 3)
        res[name] = e
        print(json.dumps({name: e}), flush=True)
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
    res["kernel_source_hash"] = bench.kernel_source_hash()
    res["commit"] = os.environ.get("LP_PROFILE_COMMIT", "")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


def save_roots(ctx, path):
    """The arguments of every workload's search (and of the warm-up's), for the processes of --ab-parent."""
    shapes = sorted({(64, 192)} | {(m, n) for m, n, _, _ in WORKLOADS.values()})
    data = {}
    for m, n in shapes:
        for k, v in enumerate(_workload(ctx, m, n)):
            data[f"{m}x{n}_{k}"] = np.asarray(v)
    np.savez(path, **data)


def solo(lib_path, snapshots, roots_path, out_path):
    """One process of --ab-parent: per workload one warm-up and one timed call of one build's entry."""
    data = np.load(roots_path)

    def args_of(m, n):
        a = [data[f"{m}x{n}_{k}"] for k in range(10)]
        return [np.asfortranarray(a[0])] + a[1:8] + [bool(a[8]), int(a[9])]

    build = Build(lib_path)
    build.solve(*args_of(64, 192), 64, 10, snapshots)
    out = {}
    for name, (m, n, depth, nodes) in WORKLOADS.items():
        args = args_of(m, n)
        build.solve(*args, depth, nodes, snapshots)
        g, ms = _clock(lambda: build.solve(*args, depth, nodes, snapshots))
        out[name] = dict(ms=ms, result=g)
    build.close()
    with open(out_path, "w") as f:
        f.write(json.dumps(out) + "\n")


def ab_parent(parent_lib, path):
    import subprocess
    import tempfile
    res = json.load(open(path)) if os.path.exists(path) else {}
    with tempfile.TemporaryDirectory() as tmp:
        roots = os.path.join(tmp, "roots.npz")
        me = [sys.executable, os.path.abspath(__file__)]
        subprocess.run(me + ["--save-roots", roots], check=True, timeout=600)
        ms = {"parent": {k: [] for k in WORKLOADS}, "k0": {k: [] for k in WORKLOADS}}
        last = {}
        for r in range(ROUNDS):
            for who, lib, snapshots in (("parent", parent_lib, "none"), ("k0", capi.lib_path(), "0")):
                out = os.path.join(tmp, f"{who}_{r}.json")
                subprocess.run(me + ["--solo", lib, snapshots, roots, out], check=True, timeout=600)
                got = json.load(open(out))
                for name in WORKLOADS:
                    ms[who][name].append(got[name]["ms"])
                last[who] = got
    for name in WORKLOADS:
        same = last["parent"][name]["result"] == last["k0"][name]["result"]
        e = dict(parent=_stats(ms["parent"][name]), k0=_stats(ms["k0"][name]), bit_equal=bool(same))
        e["k0_median_within_parent_min_max"] = bool(e["parent"]["ms_min"] <= e["k0"]["ms_median"] <= e["parent"]["ms_max"])
        e["k0_over_parent"] = round(e["k0"]["ms_median"] / e["parent"]["ms_median"], 4)
        assert same, name
        res.setdefault(name, {})["against_parent_build"] = e
        print(json.dumps({name: e}), flush=True)
    res["parent_build"] = ("lp_mip_bounded_solve_large of the parent commit's build and this build's _ex entry with 0 snapshots, "
                           f"each in a process of its own, alternated, {ROUNDS} processes of each")
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
    plib = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--ab-parent=")]
    default = os.path.join(ROOT, "profiles", "mip_bounded_snapshots.json")
    if "--trace" in sys.argv:
        add_trace(args[0], args[2] if len(args) > 2 else default, "kernels_" + args[1])
    elif plib:
        ab_parent(plib[0], args[0] if args else default)
    elif "--solo" in sys.argv:
        solo(args[0], None if args[1] == "none" else int(args[1]), args[2], args[3])
    else:
        context = capi.Context(0)
        if "--calls-only" in sys.argv:
            calls_only(context, args[0])
        elif "--save-roots" in sys.argv:
            save_roots(context, args[0])
        else:
            timed(context, args[0] if args else default)
        context.close()
