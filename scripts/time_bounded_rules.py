"""Bland's rule and Devex pricing of the bounded-variable simplex (lp_simplex_bounded_batched_ex) against Dantzig's, in
iterations and in time, on one MI355X.  Nothing here promises a speed-up: the file records what was measured.
Workloads, 4096 LPs each, seeds 0..4095, maximise: tests/bounded_ref.boxed_lp(seed, m, n, kind="box") of 32 x 96 and
64 x 192, as they are and column-scaled in the manner of tests/devex_ref.scaled_lp (structural column j of A and c_j
multiplied by s_j = 10**U(-2, 2), its bounds divided by s_j: the same vertices in other units, other reduced costs).
Per workload four variants in the same run, alternating: the Dantzig kernel through the old entry
(lp_simplex_bounded_batched), and the _ex entry under Dantzig's, Bland's and the Devex rule.  For each: the median, min
and max of 7 timed calls after one warm-up (host wall clock around the whole call: upload, kernel, download), the
iteration counts, the status histogram and the largest relative difference of the objectives against the old entry;
the first 16 LPs of every variant are checked against tests/ref/bounded_rules_ref.c bit for bit.
Kernel times do not come from this process.  `--calls-only` makes three calls per variant and workload, in the order
VARIANTS x 3 per workload, and writes nothing: the run to put under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/time_bounded_rules.py --calls-only`.
`--kernel-trace CSV` reads that run's *_kernel_trace.csv and adds kernel_ms (median, min, max of the three dispatches)
to each variant, after checking that every dispatch ran the kernel the variant names.
Writes profiles/bounded_rules.json (or the path given as the first argument) and prints it."""
import collections
import csv
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
from tests import bounded_ref as B  # noqa: E402
from tests import bounded_rules_ref as R  # noqa: E402

BATCH, REF_CHECKED, RUNS, TRACE_CALLS = 4096, 16, 7, 3
SHAPES = ((32, 96), (64, 192))
NAMES = {0: "optimal", 1: "unbounded", 2: "iter_limit", 3: "singular", 4: "infeasible", 5: "bad_arg"}
# (name, pivot_rule keyword, the kernel's name up to its template arguments)
VARIANTS = (("dantzig_old_entry", None, "k_batched_bounded"), ("dantzig_ex", R.DANTZIG, "k_batched_bounded"),
            ("bland_ex", R.BLAND, "k_batched_bounded_bland"), ("devex_ex", R.DEVEX, "k_batched_bounded_devex"))
KERNEL = re.compile(r"\d*(k_batched_bounded\w*?)(<|ILi)")   # demangled or mangled


def workload(m, n, scaled, batch=BATCH):
    cases = [B.boxed_lp(k, m, n, maximize=True, kind="box")[:5] for k in range(batch)]
    A, b, c, lo, hi = (np.stack([cs[i] for cs in cases]) for i in range(5))
    if scaled:
        for k in range(batch):
            s = 10.0 ** np.random.default_rng(k).uniform(-2.0, 2.0, n - m)
            A[k][:, :n - m] *= s
            c[k][:n - m] *= s
            lo[k][:n - m] /= s
            hi[k][:n - m] /= s
    return A, b, c, lo, hi


def workloads(batch=BATCH):
    for m, n in SHAPES:
        for scaled in (False, True):
            yield f"boxed_{m}x{n}" + ("_scaled" if scaled else ""), m, n, workload(m, n, scaled, batch)


def _hist(status):
    return dict(sorted(collections.Counter(NAMES[int(s)] for s in status).items()))


def kernel_times(path):
    """{(workload, variant): [ms, ms, ms]} from a rocprofv3 kernel trace of a --calls-only run."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if KERNEL.search(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = [(f"boxed_{m}x{n}" + ("_scaled" if scaled else ""), v) for m, n in SHAPES for scaled in (False, True)
             for v in VARIANTS for _ in range(TRACE_CALLS)]
    if len(rows) != len(order):
        raise SystemExit(f"{path}: {len(rows)} bounded dispatches, expected {len(order)}")
    out = collections.defaultdict(list)
    for r, (wl, (name, _, kernel)) in zip(rows, order):
        if KERNEL.search(r["Kernel_Name"]).group(1) != kernel:
            raise SystemExit(f"{path}: {wl} {name} ran {r['Kernel_Name']}, expected {kernel}")
        out[(wl, name)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    return out


def main(path, calls_only=False, trace=None, batch=BATCH):
    kern = kernel_times(trace) if trace else {}
    ctx = capi.Context(0)
    res = {"scenario": f"{batch} x boxed_lp(seed, m, n, kind='box'), maximise, as generated and with the structural "
                       "columns scaled by 10**U(-2, 2); lp_simplex_bounded_batched (the Dantzig kernel through the old "
                       "entry) and lp_simplex_bounded_batched_ex under each rule in the same run, alternating; call_ms: "
                       f"host wall clock of the whole call, median of {RUNS} after a warm-up; kernel_ms: rocprofv3 "
                       f"--kernel-trace over {TRACE_CALLS} calls per variant in a run of its own",
           "runs": RUNS}
    for wl, m, n, (A, b, c, lo, hi) in workloads(batch):
        def call(rule):
            return ctx.bounded_batched(A, b, c, lo, hi, True, n - m, pivot_rule=rule)

        if calls_only:
            for _, rule, _ in VARIANTS:
                for _ in range(TRACE_CALLS):
                    call(rule)
            continue
        outs = {name: call(rule) for name, rule, _ in VARIANTS}   # warm-up
        ms = {name: [] for name, _, _ in VARIANTS}
        for _ in range(RUNS):
            for name, rule, _ in VARIANTS:
                t0 = time.perf_counter()
                call(rule)
                ms[name].append((time.perf_counter() - t0) * 1e3)
        base = outs["dantzig_old_entry"]
        entry = dict(shape=f"{m}x{n}", lps=batch)
        for name, rule, _ in VARIANTS:
            o, it = outs[name], outs[name]["iters"]
            for k in range(min(REF_CHECKED, batch)):
                r = R.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n - m, rule=rule or R.DANTZIG)
                assert int(o["status"][k]) == r["status"] and [int(v) for v in it[k]] == r["iters"], (wl, name, k)
                assert np.array_equal(o["basis"][k], r["basis"]) and (r["status"] or o["obj"][k] == r["obj"]), (wl, name, k)
            ok = (o["status"] == 0) & (base["status"] == 0)
            rel = np.abs(o["obj"][ok] - base["obj"][ok]) / np.maximum(1.0, np.abs(base["obj"][ok]))
            v = dict(call_ms_median=round(float(np.median(ms[name])), 3), call_ms_min=round(min(ms[name]), 3),
                     call_ms_max=round(max(ms[name]), 3), pivots_phase1=int(it[:, 0].sum()),
                     pivots_driveout=int(it[:, 1].sum()), pivots_phase2=int(it[:, 2].sum()), flips=int(it[:, 3].sum()),
                     iterations=int(it.sum()), status=_hist(o["status"]),
                     status_mismatches_vs_old_entry=int((o["status"] != base["status"]).sum()),
                     max_rel_obj_diff_vs_old_entry=float(rel.max()) if rel.size else 0.0)
            if (wl, name) in kern:
                k3 = kern[(wl, name)]
                v.update(kernel_ms_median=round(float(np.median(k3)), 4), kernel_ms_min=round(min(k3), 4),
                         kernel_ms_max=round(max(k3), 4))
            entry[name] = v
        same = all(np.array_equal(outs["dantzig_ex"][key], base[key]) for key in ("status", "basis", "at_upper", "iters"))
        entry["dantzig_ex_equals_old_entry"] = bool(same and np.array_equal(outs["dantzig_ex"]["x"], base["x"],
                                                                            equal_nan=True))
        for name in ("bland_ex", "devex_ex"):
            entry[name]["iterations_over_dantzig"] = round(entry[name]["iterations"] /
                                                           entry["dantzig_old_entry"]["iterations"], 3)
            if "kernel_ms_median" in entry[name]:
                entry[name]["kernel_ms_over_dantzig"] = round(entry[name]["kernel_ms_median"] /
                                                              entry["dantzig_old_entry"]["kernel_ms_median"], 3)
        res[wl] = entry
    ctx.close()
    if calls_only:
        return
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    trace = batch = None
    if "--kernel-trace" in argv:
        i = argv.index("--kernel-trace")
        trace = argv[i + 1]
        del argv[i:i + 2]
    if "--batch" in argv:   # a smaller batch, for a rehearsal
        i = argv.index("--batch")
        batch = int(argv[i + 1])
        del argv[i:i + 2]
    args = [a for a in argv if a != "--calls-only"]
    main(args[0] if args else os.path.join(ROOT, "profiles", "bounded_rules.json"), "--calls-only" in argv, trace,
         batch or BATCH)
