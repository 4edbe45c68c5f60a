"""The dual ratio test of the branch-and-bound over the bounds (LP_DUAL_RATIO_TEXTBOOK against
LP_DUAL_RATIO_LONG_STEP) on the GPU, whole calls.
Workloads:
  LDS, lp_mip_bounded_solve_batched_ratio_ex (scripts/time_mip_bounded.py's batches of 4096, and one more)
    boxed_32x96_d64, boxed_32x96_d256   boxed_lp(k, 32, 96, kind="box"), the 64 structural columns integer with hi
                                        rounded up, from a cold lp_simplex_bounded_batched, max_nodes 2000
    rows_16x40_d24, rows_16x40_d256     gen_lp(k, 16, 40), the 24 original columns integer, slack bases, lo = 0,
                                        hi = inf (the only finite boxes are those the branches make), max_nodes 2000
    boxed_64x192_d64                    boxed_lp(k, 64, 192, kind="box") the same way, max_nodes 500
  HBM, lp_mip_bounded_solve_large_ratio_ex (scripts/time_mip_bounded_snapshots.py's problems: boxed_mip(1, m, n, "mixed",
  every=2) from the Devex root of lp_simplex_bounded_large_ex), each with 0 and 4 snapshots
    512x1024_200       max_depth 64, 200 nodes
    2048x4096_rebuild  max_depth 4, 32 nodes
Per workload one warm-up of each ratio test, then ROUNDS alternated rounds in one session: host wall clock of the whole
call (upload, every launch, download; it ends in a device synchronise) as median, min and max; nodes, dual pivots,
flips, and the problems closed (the search ended LP_OPTIMAL or LP_INFEASIBLE under the same max_nodes).

The guard (--parent-lib=PATH): within the same rounds, one fresh process per round and build times the parent build's
entries without a suffix and this build's _ratio_ex entries under LP_DUAL_RATIO_TEXTBOOK (the order alternates by round)
on the same workloads, each after one untimed call.  `textbook_within_parent` says whether the new entry's median is no
slower than the parent's slowest run, `outputs_equal` whether every output of the two agrees bit for bit.

  python scripts/time_mip_bounded_long_step.py [--parent-lib=PATH] [out.json]
                                      the timed run; writes profiles/mip_bounded_long_step.json"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = int(os.environ.get("LP_TIME_BATCH", "4096"))
ROUNDS = int(os.environ.get("LP_TIME_ROUNDS", "5"))
MAX_ITER = 1000000
# name -> (kind, m, n, max_depth, max_nodes)
LDS = {"boxed_32x96_d64": ("box", 32, 96, 64, 2000), "boxed_32x96_d256": ("box", 32, 96, 256, 2000),
       "rows_16x40_d24": ("rows", 16, 40, 24, 2000), "rows_16x40_d256": ("rows", 16, 40, 256, 2000),
       "boxed_64x192_d64": ("box", 64, 192, 64, 500)}
# name -> (m, n, max_depth, max_nodes, snapshots)
HBM = {"512x1024_200_k0": (512, 1024, 64, 200, 0), "512x1024_200_k4": (512, 1024, 64, 200, 4),
       "2048x4096_rebuild_k0": (2048, 4096, 4, 32, 0), "2048x4096_rebuild_k4": (2048, 4096, 4, 32, 4)}
if os.environ.get("LP_TIME_SMALL"):   # a rehearsal at toy sizes
    HBM = {"96x192_k0": (96, 192, 8, 20, 0), "96x192_k4": (96, 192, 8, 20, 4)}


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def _digest(out):
    h = hashlib.sha256()
    for k in ("status", "found", "x", "obj", "bound", "stats"):
        h.update(np.ascontiguousarray(np.asarray(out[k])).tobytes())
    return h.hexdigest()[:16]


def _counts(out):
    st, s = np.atleast_1d(out["status"]), np.atleast_2d(np.asarray(out["stats"]))
    return dict(nodes=int(s[:, 0].sum()), dual_pivots=int(s[:, 1].sum()), primal_pivots=int(s[:, 2].sum()),
                flips=int(s[:, 3].sum()), closed=int(((st == 0) | (st == 4)).sum()), problems=int(len(st)))


_lds_cache = {}


def lds_batch(ctx, capi, kind, m, n):
    """The batch and its starts: (A, b, c, lo, hi, mask, basis, at_upper)."""
    from tests import bounded_ref
    if (kind, m, n) in _lds_cache:
        return _lds_cache[(kind, m, n)]
    no = n - m
    A, b, c = np.empty((BATCH, m, n)), np.empty((BATCH, m)), np.empty((BATCH, n))
    mask = np.r_[np.ones(no), np.zeros(m)].astype(np.int32)
    if kind == "rows":
        basis = np.empty((BATCH, m), np.int32)
        for k in range(BATCH):
            A[k], b[k], c[k], basis[k] = capi.gen_lp(k, m, n)
        lo, hi, up = np.zeros((BATCH, n)), np.full((BATCH, n), np.inf), np.zeros((BATCH, n), np.int32)
    else:
        lo, hi = np.empty((BATCH, n)), np.empty((BATCH, n))
        for k in range(BATCH):
            A[k], b[k], c[k], lo[k], hi[k], _ = bounded_ref.boxed_lp(k, m, n, maximize=True, kind="box")
        hi[:, :no] = np.ceil(hi[:, :no])
        cold = ctx.bounded_batched(A, b, c, lo, hi, True, no, max_iter=MAX_ITER)
        ok = cold["status"] == 0
        basis, up = np.where(ok[:, None], cold["basis"], 0), np.where(ok[:, None], cold["at_upper"], 0)
        hi = np.where(ok[:, None], hi, lo)   # (an LP whose cold solve failed: fixed, one node)
    _lds_cache[(kind, m, n)] = (A, b, c, lo, hi, mask, basis, up)
    return _lds_cache[(kind, m, n)]


def lds_call(ctx, capi, name, dual_ratio):
    kind, m, n, depth, nodes = LDS[name]
    A, b, c, lo, hi, mask, basis, up = lds_batch(ctx, capi, kind, m, n)
    return ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, maximize=True, n_orig=n - m, max_depth=depth,
                                         max_nodes=nodes, max_iter=MAX_ITER, dual_ratio=dual_ratio)


_roots = {}


def hbm_root(ctx, capi, m, n):
    from tests import mip_bounded_ref as R
    if (m, n) not in _roots:
        A, b, c, lo, hi, mask, mx = R.boxed_mip(1, m, n, None, "mixed", 2)
        A = np.asfortranarray(A)   # the ABI's layout: no variant pays a transpose per call
        root = ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=MAX_ITER, pivot_rule=capi.PIVOT_DEVEX)
        assert root["status"] == 0, root["status"]
        _roots[(m, n)] = (A, b, c, lo, hi, root["basis"], root["at_upper"], mask, mx, n - m)
    return _roots[(m, n)]


def hbm_call(ctx, args, name, dual_ratio):
    m, n, depth, nodes, K = HBM[name]
    return ctx.mip_bounded_solve_large(*args, max_depth=depth, max_nodes=nodes, max_iter=MAX_ITER, snapshots=K,
                                       dual_ratio=dual_ratio)


# ---- the guard: a fresh process per round and build --------------------------------------------------------------
def guard_child(path, parent, npz):
    """One process of the guard on the library at `path`: every workload once after one untimed call; one JSON line.
    parent: the entries without a suffix (the build has no others); else the _ratio_ex entries under TEXTBOOK."""
    os.environ["LP_LIB_PATH"] = path
    from simplexmethod_amd import capi
    if parent:
        for name in [k for k in capi.SIGNATURES if k.startswith("lp_mip_bounded_solve") and k.endswith("_ratio_ex")]:
            del capi.SIGNATURES[name]
    ratio = None if parent else "textbook"
    ctx = capi.Context(0)
    data = np.load(npz)
    out = {}
    for name in LDS:
        lds_call(ctx, capi, name, ratio)
        g, t = _clock(lambda: lds_call(ctx, capi, name, ratio))
        out[name] = dict(ms=t, digest=_digest(g), **_counts(g))
    for name, (m, n, _, _, _) in HBM.items():
        a = [data[f"{m}x{n}_{k}"] for k in range(10)]
        args = [np.asfortranarray(a[0])] + a[1:8] + [bool(a[8]), int(a[9])]
        hbm_call(ctx, args, name, ratio)
        g, t = _clock(lambda: hbm_call(ctx, args, name, ratio))
        out[name] = dict(ms=t, digest=_digest(g), **_counts(g))
    ctx.close()
    print("GUARD " + json.dumps(out), flush=True)


def _guard_round(npz, parent_lib, own_lib, k):
    res = {}
    builds = [("new_textbook", own_lib, 0), ("parent", parent_lib, 1)]
    for label, path, parent in (builds if k % 2 == 0 else builds[::-1]):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child", path, str(parent), npz],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"guard child {label} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("GUARD ")][-1]
        res[label] = json.loads(line[6:])
    return res


# ---- the timed run -------------------------------------------------------------------------------------------
def timed(parent_lib, path):
    import bench  # (kernel_source_hash)
    from simplexmethod_amd import capi
    ctx = capi.Context(0)
    res = {"scenario": f"{ROUNDS} alternated rounds in one session after one warm-up of each; host wall clock of the "
                       "whole call; LP_DUAL_RATIO_TEXTBOOK and LP_DUAL_RATIO_LONG_STEP through the _ratio_ex entries "
                       f"of the search over the bounds; LDS batches of {BATCH}",
           "guard": "a fresh process per round and build, within the same rounds" if parent_lib else
                    "not measured (no --parent-lib)"}
    runs = {}
    for name in LDS:
        runs[name] = {r: (lambda name=name, r=r: lds_call(ctx, capi, name, r)) for r in ("textbook", "long_step")}
    for name, (m, n, _, _, _) in HBM.items():
        args = hbm_root(ctx, capi, m, n)
        runs[name] = {r: (lambda args=args, name=name, r=r: hbm_call(ctx, args, name, r)) for r in ("textbook", "long_step")}
    tmp = tempfile.mkdtemp(prefix="lp_mip_long_step_")
    npz = os.path.join(tmp, "roots.npz")
    if parent_lib:
        np.savez(npz, **{f"{m}x{n}_{k}": np.asarray(v) for (m, n), a in _roots.items() for k, v in enumerate(a)})
    for name in runs:   # warm-up: code objects, the context's pools, every shape
        for fn in runs[name].values():
            fn()
        print(f"warmed {name}", file=sys.stderr, flush=True)
    ms = {k: {v: [] for v in runs[k]} for k in runs}
    out = {k: {} for k in runs}
    guard = []
    for k in range(ROUNDS):
        print(f"round {k + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        for name in runs:
            for v, fn in runs[name].items():
                out[name][v], t = _clock(fn)
                ms[name][v].append(t)
        if parent_lib:
            guard.append(_guard_round(npz, parent_lib, capi.lib_path(), k))
    if parent_lib:
        os.remove(npz)
    os.rmdir(tmp)
    for name in runs:
        e = dict(workload=LDS.get(name) or HBM[name])
        for v in runs[name]:
            e[v] = dict(_stats(ms[name][v]), **_counts(out[name][v]))
        a, g = out[name]["textbook"], out[name]["long_step"]
        sa, sg = np.atleast_1d(a["status"]), np.atleast_1d(g["status"])
        both = (sa == 0) & (sg == 0)
        za, zg = np.atleast_1d(a["obj"])[both], np.atleast_1d(g["obj"])[both]
        e["both_optimal"] = int(both.sum())
        e["objectives_agree"] = bool(np.all(np.abs(za - zg) <= 1e-9 + 1e-9 * np.abs(za)))
        ta, tg = e["textbook"], e["long_step"]
        e["speedup_long_step"] = round(ta["ms_median"] / tg["ms_median"], 3)
        # the medians separate beyond the rounds' spread when the two min-max ranges do not overlap
        e["separated"] = bool(tg["ms_max"] < ta["ms_min"] or ta["ms_max"] < tg["ms_min"])
        if guard:
            new = _stats([g_["new_textbook"][name]["ms"] for g_ in guard])
            old = _stats([g_["parent"][name]["ms"] for g_ in guard])
            same = all(g_["new_textbook"][name]["digest"] == g_["parent"][name]["digest"] for g_ in guard)
            e["guard"] = dict(new_textbook=new, parent=old, outputs_equal=bool(same),
                              textbook_within_parent=bool(new["ms_median"] <= old["ms_max"]))
        res[name] = e
        print(json.dumps({name: e}), flush=True)
    res["kernel_source_hash"] = bench.kernel_source_hash()
    res["commit"] = os.environ.get("LP_PROFILE_COMMIT", "")
    ctx.close()
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    plib = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parent-lib=")]
    default = os.path.join(ROOT, "profiles", "mip_bounded_long_step.json")
    if "--guard-child" in sys.argv:
        guard_child(args[0], int(args[1]), args[2])
    else:
        timed(os.path.abspath(plib[0]) if plib else None, args[0] if args else default)
