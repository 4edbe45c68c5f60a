"""The dual ratio test of the bounded re-solve (LP_DUAL_RATIO_TEXTBOOK against LP_DUAL_RATIO_LONG_STEP) on the GPU,
under each dual rule.
Workloads (those of scripts/time_bounded_resolve_dual_rules.py):
  - tests/bounded_ref.boxed_lp(1, m, n, kind="box") at 512 x 1024 and 2048 x 4096, cold-solved by
    lp_simplex_bounded_large_ex under Devex, then three bounds of basic columns tightened
    (tests/bounded_resolve_ref.perturb, "bound": the first seed that changes three bounds and whose warm result is
    optimal).  ROUNDS alternated rounds in one session of lp_simplex_bounded_resolve_large_ratio_ex under the four
    (dual rule, ratio test) pairs: host wall clock of the whole call (upload, every launch, download; ends in a device
    synchronise) as median, min and max, the dual pivots and flips, and the objectives' agreement;
  - the batch: 4096 boxed LPs of 64 x 192 (boxed_lp(seed, 64, 192, kind="mixed")), cold-solved by
    lp_simplex_bounded_batched, one to three bounds tightened each; lp_simplex_bounded_resolve_batched_ratio_ex in the
    same alternated way, with the pivots and flips summed over the batch.
The guard (--parent-lib=PATH): within the same rounds, one fresh process per round times this build's _ratio_ex entries
under LP_DUAL_RATIO_TEXTBOOK, another the parent build's _dual_ex entries and a third this build's own _dual_ex entries
(the same kernels as the first: what two processes of one build differ by; the order of the three rotates by round),
on the same saved warm starts under both dual rules, each entry warmed by one untimed call at its shape.
`textbook_within_parent` says whether each median of the new entry is no slower than the parent's slowest run, and
`self_within_parent` the same of this build's _dual_ex entries.

  python scripts/time_bounded_resolve_long_step.py [--parent-lib=PATH] [out.json]
                                      the timed run; writes profiles/bounded_resolve_long_step.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_bounded_resolve_long_step.py --calls-only DIR/calls.json
                                      one warm call per shape, dual rule and ratio test, in an order calls.json records
  python scripts/time_bounded_resolve_long_step.py --trace DIR [out.json]
      adds to out.json, per shape, dual rule and ratio test, the mean and median duration of the dual selector over the
      launches that staged a pivot, and the summed duration of every kernel of the call."""
import csv
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
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
RULES = (("dantzig", capi.DUAL_DANTZIG), ("devex", capi.DUAL_DEVEX))
RATIOS = (("textbook", capi.DUAL_RATIO_TEXTBOOK), ("long_step", capi.DUAL_RATIO_LONG_STEP))


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


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


# ---- the guard: a fresh process per round and build --------------------------------------------------------------
class Raw:
    """The re-solve entries of one build of the library through ctypes alone: this build's _ratio_ex entries under
    LP_DUAL_RATIO_TEXTBOOK, or (parent) another build's _dual_ex entries."""

    def __init__(self, path, parent):
        self.lib, self.parent = C.CDLL(path), parent
        self.suffix = "_dual_ex" if parent else "_ratio_ex"
        for name in ("lp_context_create", "lp_context_destroy"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = capi.SIGNATURES[name]
        for name in ("lp_simplex_bounded_resolve_large", "lp_simplex_bounded_resolve_batched"):
            fn = getattr(self.lib, name + self.suffix)
            fn.restype, fn.argtypes = capi.SIGNATURES[name + self.suffix]
        self.h = C.c_void_p()
        assert self.lib.lp_context_create(0, None, C.byref(self.h)) == 0

    def close(self):
        self.lib.lp_context_destroy(self.h)

    def _tail(self, dual_rule):
        return (capi.PIVOT_DANTZIG, dual_rule) if self.parent else (capi.PIVOT_DANTZIG, dual_rule, capi.DUAL_RATIO_TEXTBOOK)

    def resolve_large(self, start, maximize, n_orig, dual_rule):
        p = capi.pack_lp(*start[:3], start[5], start[3], start[4], start[6])
        x, bo, uo = np.full(n_orig, np.nan), np.zeros(p.m, np.int32), np.zeros(p.n, np.int32)
        obj, it = np.full(1, np.nan), np.zeros(3, np.int32)
        d, i = capi._d, capi._i
        fn = getattr(self.lib, "lp_simplex_bounded_resolve_large" + self.suffix)
        st = fn(self.h, d(p.A), p.m, p.n, d(p.b), d(p.c), d(p.lo), d(p.hi), i(p.basis), i(p.at_upper), int(maximize),
                n_orig, capi.EPS, MAX_ITER, d(x), i(bo), i(uo), d(obj), i(it), *self._tail(dual_rule))
        return dict(status=st, obj=float(obj[0]), iters=it.tolist())

    def resolve_batched(self, start, maximize, n_orig, dual_rule):
        p = capi.pack_lp(*start[:3], start[5], start[3], start[4], start[6], batched=True)
        B = p.batch
        x, bo, uo = np.full((B, n_orig), np.nan), np.zeros((B, p.m), np.int32), np.zeros((B, p.n), np.int32)
        obj, it, st = np.full(B, np.nan), np.zeros((B, 3), np.int32), np.zeros(B, np.int32)
        d, i = capi._d, capi._i
        fn = getattr(self.lib, "lp_simplex_bounded_resolve_batched" + self.suffix)
        rc = fn(self.h, B, d(p.A), p.m, p.n, d(p.b), d(p.c), d(p.lo), d(p.hi), i(p.basis), i(p.at_upper), int(maximize),
                n_orig, capi.EPS, MAX_ITER, d(x), i(bo), i(uo), d(obj), i(it), i(st), *self._tail(dual_rule))
        assert rc == 0
        return dict(iters=[int(v) for v in it.sum(axis=0)])


def guard_child(path, parent, npz):
    """One process of the guard: every saved warm start once under each dual rule, each after one untimed call of the
    same entry at the same shape (code objects, the context's pools); one JSON line."""
    raw = Raw(path, parent)
    data = np.load(npz)
    starts = {k: tuple(data[f"{k}_{i}"] for i in range(7)) for k in json.loads(str(data["keys"]))}
    out = {}
    for key, start in starts.items():
        if key == "batch":
            call = lambda rule: raw.resolve_batched(start, True, BN - BM, rule)   # noqa: E731
        else:
            m, n = start[0].shape
            call = lambda rule: raw.resolve_large(start, bool(data[key + "_mx"]), n - m, rule)   # noqa: E731
        call(capi.DUAL_DANTZIG)
        for name, rule in RULES:
            g, t = _clock(lambda: call(rule))
            out[f"{key}/{name}"] = dict(ms=t, iters=g["iters"])
    raw.close()
    print("GUARD " + json.dumps(out), flush=True)


def _guard_round(npz, parent_lib, k):
    res = {}
    builds = [("new_textbook", capi.lib_path(), 0), ("parent_dual_ex", parent_lib, 1), ("self_dual_ex", capi.lib_path(), 1)]
    for label, path, parent in builds[k % 3:] + builds[:k % 3]:   # (the order rotates by round)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child", path, str(parent), npz],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"guard child {label} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("GUARD ")][-1]
        res[label] = json.loads(line[6:])
    return res


# ---- the timed run -------------------------------------------------------------------------------------------
def timed(ctx, parent_lib, path):
    res = {"scenario": f"{ROUNDS} alternated rounds in one session; host wall clock of the whole call; the dual ratio "
                       "tests LP_DUAL_RATIO_TEXTBOOK and LP_DUAL_RATIO_LONG_STEP of the bounded re-solve under each "
                       "dual rule",
           "guard": "a fresh process per round and build, within the same rounds" if parent_lib else
                    "not measured (no --parent-lib)"}
    A, b, c, lo, hi, mx = R.boxed_lp(1, 64, 192, kind="mixed")   # warm-up: code objects, the context's pools
    w = ctx.bounded_large(A, b, c, lo, hi, mx)
    for _, rule in RULES:
        for _, ratio in RATIOS:
            ctx.bounded_resolve_large(A, b, c, lo, hi, w["basis"], w["at_upper"], mx, dual_rule=rule, dual_ratio=ratio)
            ctx.bounded_resolve(A, b, c, lo, hi, w["basis"], w["at_upper"], mx, dual_rule=rule, dual_ratio=ratio)
    work, runs, meta, sense = {}, {}, {}, {"batch": True}
    for m, n in SHAPES:
        start, mx, pseed, boxes, cold = _workload(ctx, m, n)
        key = f"boxed_{m}x{n}"
        work[key], sense[key] = start, bool(mx)
        meta[key] = dict(shape=f"{m}x{n}", boxes=boxes, perturb_seed=pseed, bounds_changed=3, crash_pivots=m,
                         cold_devex_iters=cold["iters"])
        runs[key] = {f"{rn}/{qn}": (lambda s=start, mx=mx, k=n - m, r=rule, q=ratio: ctx.bounded_resolve_large(
            *s, mx, k, max_iter=MAX_ITER, dual_rule=r, dual_ratio=q)) for rn, rule in RULES for qn, ratio in RATIOS}
    bstart, keep = _batch_workload(ctx)
    work["batch"] = bstart
    meta["batch"] = dict(shape=f"{BATCH} x {BM}x{BN}", cold_optimal=int(len(keep)))
    runs["batch"] = {f"{rn}/{qn}": (lambda r=rule, q=ratio: ctx.bounded_resolve_batched(
        *bstart, True, BN - BM, max_iter=MAX_ITER, dual_rule=r, dual_ratio=q)) for rn, rule in RULES for qn, ratio in RATIOS}
    tmp = tempfile.mkdtemp(prefix="lp_long_step_")
    npz = os.path.join(tmp, "starts.npz")
    if parent_lib:
        arrays = {f"{k}_{i}": np.asarray(s[i]) for k, s in work.items() for i in range(7)}
        np.savez(npz, keys=json.dumps(list(work)), **{f"{k}_mx": v for k, v in sense.items()}, **arrays)
    ms = {k: {v: [] for v in runs[k]} for k in runs}
    out = {k: {} for k in runs}
    guard = []
    for k in range(ROUNDS):
        print(f"round {k + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        for key in runs:
            for v, fn in runs[key].items():
                out[key][v], t = _clock(fn)
                ms[key][v].append(t)
        if parent_lib:
            guard.append(_guard_round(npz, parent_lib, k))
    if parent_lib:
        os.remove(npz)
    os.rmdir(tmp)
    for key in runs:
        e = meta[key]
        for v in runs[key]:
            o = out[key][v]
            if key == "batch":
                st, it = np.asarray(o["status"])[keep], np.asarray(o["iters"])[keep]
                e[v] = dict(_stats(ms[key][v]), optimal=int((st == 0).sum()), infeasible=int((st == 4).sum()),
                            dual_pivots=int(it[:, 0].sum()), flips=int(it[:, 2].sum()))
            else:
                e[v] = dict(_stats(ms[key][v]), status=int(o["status"]), dual_pivots=int(o["iters"][0]),
                            flips=int(o["iters"][2]), obj=o["obj"])
        for rn, _ in RULES:
            a, g = out[key][f"{rn}/textbook"], out[key][f"{rn}/long_step"]
            if key == "batch":
                sa, sg = np.asarray(a["status"]), np.asarray(g["status"])
                ok = keep[(sa[keep] == 0) & (sg[keep] == 0)]
                za, zg = np.asarray(a["obj"])[ok], np.asarray(g["obj"])[ok]
                e[f"{rn}/statuses_agree"] = bool(np.array_equal(sa, sg))
                e[f"{rn}/objectives_agree"] = bool(np.all(np.abs(za - zg) <= 1e-7 * np.maximum(1.0, np.abs(za))))
            else:
                e[f"{rn}/objectives_agree"] = bool(a["status"] == g["status"] == 0 and
                                                   abs(a["obj"] - g["obj"]) <= 1e-7 * max(1.0, abs(a["obj"])))
            ta, tg = e[f"{rn}/textbook"], e[f"{rn}/long_step"]
            e[f"{rn}/speedup_long_step"] = round(ta["ms_median"] / tg["ms_median"], 3)
            # the medians separate beyond the rounds' spread when the two min-max ranges do not overlap
            e[f"{rn}/separated"] = bool(tg["ms_max"] < ta["ms_min"] or ta["ms_max"] < tg["ms_min"])
            if guard:
                new = _stats([g_["new_textbook"][f"{key}/{rn}"]["ms"] for g_ in guard])
                old = _stats([g_["parent_dual_ex"][f"{key}/{rn}"]["ms"] for g_ in guard])
                own = _stats([g_["self_dual_ex"][f"{key}/{rn}"]["ms"] for g_ in guard])
                same = all(g_["new_textbook"][f"{key}/{rn}"]["iters"] == g_["parent_dual_ex"][f"{key}/{rn}"]["iters"] for g_ in guard)
                e[f"{rn}/guard"] = dict(new_textbook=new, parent_dual_ex=old, self_dual_ex=own, counts_equal=bool(same),
                                        textbook_within_parent=bool(new["ms_median"] <= old["ms_max"]),
                                        self_within_parent=bool(own["ms_median"] <= old["ms_max"]))
        res[key] = e
        print(json.dumps({key: e}), flush=True)
    res["kernel_source_hash"] = bench.kernel_source_hash()
    res["commit"] = os.environ.get("LP_PROFILE_COMMIT", "")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


# ---- the kernel trace ----------------------------------------------------------------------------------------
def calls_only(ctx, side):
    order = []

    def note(label, **kw):
        order.append(dict(label=label, **kw))
        with open(side, "w") as f:   # (after every call: a run cut short still says what it traced)
            json.dump(order, f)

    for m, n in SHAPES:
        start, mx, _, _, cold = _workload(ctx, m, n)
        note(f"setup/{m}x{n}", uploads=1 + cold["warm_tries"])   # the cold call and one warm call per perturbation tried
        for rn, rule in RULES:
            for qn, ratio in RATIOS:
                g = ctx.bounded_resolve_large(*start, mx, n - m, max_iter=MAX_ITER, dual_rule=rule, dual_ratio=ratio)
                note(f"{rn}/{qn}/{m}x{n}", uploads=1, iters=g["iters"], status=int(g["status"]))


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
        if entry["label"].startswith("setup/"):
            continue
        rn, qn, shape = entry["label"].split("/")
        ks, live = calls[pos - 1], entry["iters"][0]   # (every dual pivot is one selector launch; flips ride in them)
        sel = [d for q, d in ks if "k_simplex_select_dual_bounded" in q][:live]
        kern = sorted({re.search(r"k_simplex_select_dual_bounded\w*", q).group(0) for q, _ in ks
                       if "k_simplex_select_dual_bounded" in q})
        res.setdefault(f"boxed_{shape}", {}).setdefault("kernel_trace", {})[f"{rn}/{qn}"] = dict(
            kernel=kern, iters=entry["iters"], status=entry["status"], pivots_in_trace=len(sel),
            select_us_mean=round(float(np.mean(sel)), 2) if sel else None,
            select_us_median=round(float(np.median(sel)), 2) if sel else None,
            kernels_ms_sum=round(sum(d for _, d in ks) * 1e-3, 3), launches=len(ks))
        print(shape, rn, qn, json.dumps(res[f"boxed_{shape}"]["kernel_trace"][f"{rn}/{qn}"]), flush=True)
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    plib = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parent-lib=")]
    default = os.path.join(ROOT, "profiles", "bounded_resolve_long_step.json")
    if "--guard-child" in sys.argv:
        guard_child(args[0], int(args[1]), args[2])
    elif "--trace" in sys.argv:
        add_trace(args[0], args[1] if len(args) > 1 else default)
    else:
        context = capi.Context(0)
        if "--calls-only" in sys.argv:
            calls_only(context, args[0] if args else "calls.json")
        else:
            timed(context, os.path.abspath(plib[0]) if plib else None, args[0] if args else default)
        context.close()
