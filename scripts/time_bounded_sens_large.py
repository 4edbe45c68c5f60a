"""Time of the dual solution and of RHS / cost ranging of a bounded-variable LP beyond one workgroup's LDS
(lp_basis_bounded_duals_large, lp_basis_bounded_ranging_large) at the optimum lp_simplex_bounded_large_ex returns.
Workloads: tests/bounded_ref.boxed_lp(1, m, n, kind="mixed") at 512 x 1024 and 2048 x 4096, cold-solved under
LP_PIVOT_DEVEX.  Then ROUNDS alternated rounds in one session, after one warm-up round, of
  (a) lp_basis_bounded_duals_large,
  (b) lp_basis_bounded_ranging_large,
  (c) lp_basis_ranging on the same A and basis (lo = 0, hi = inf: the plain HBM path, which does the same two crashes
      and the same B^-1 A): the yardstick of (b),
each as host wall clock of the whole call (upload, every launch, download; ends in a device synchronise): median, min
and max.  (d) is tests/ref/bounded_sens_ref.c on one core, duals and ranging once each; (a) and (b) are compared with it
bit for bit.  Also recorded: w against the solver's objective, and that every b_i and c_j lies in its own range.

  python scripts/time_bounded_sens_large.py [out.json]      the timed run; writes profiles/bounded_sens_large.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_bounded_sens_large.py --calls-only
      the solve and (a), (b), (c) once per shape, nothing written: the kernels' own durations"""
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
from tests import bounded_sens_ref as S  # noqa: E402

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
    """The LP, its Devex optimum, and the three calls at that basis."""
    A, b, c, lo, hi, mx = R.boxed_lp(1, m, n, kind="mixed")
    sol = ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=MAX_ITER, pivot_rule="devex")
    assert sol["status"] == 0 and sol["basis"].max() < n, sol["status"]
    at = (A, b, c, lo, hi, sol["basis"], sol["at_upper"])
    calls = dict(duals_large=lambda: ctx.bounded_duals_large(*at),
                 ranging_large=lambda: ctx.bounded_ranging_large(*at, mx),
                 plain_ranging=lambda: ctx.basis_ranging(A, b, c, sol["basis"], mx))
    return at, mx, sol, calls


def main(path, calls_only=False):
    ctx = capi.Context(0)
    res = {"scenario": "boxed_lp(1, m, n, 'mixed') solved by lp_simplex_bounded_large_ex under LP_PIVOT_DEVEX, analysed at "
                       f"its basis and flags; {ROUNDS} alternated rounds in one session after a warm-up round; host wall "
                       "clock of the whole call; plain_ranging is lp_basis_ranging on the same A and basis; the "
                       "reference is tests/ref/bounded_sens_ref.c on one core, once"}
    for m, n in SHAPES:
        at, mx, sol, calls = _workload(ctx, m, n)
        out = {k: fn() for k, fn in calls.items()}   # warm-up: code objects, the first allocations of this size
        if calls_only:
            continue
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                out[k], t = _clock(fn)
                ms[k].append(t)
        g, q = out["duals_large"], out["ranging_large"]
        rg, ref_d_ms = _clock(lambda: S.duals(*at))
        rq, ref_r_ms = _clock(lambda: S.ranging(*at, mx))
        assert g["status"] == rg["status"] == 0 and q["status"] == rq["status"] == 0
        S.same_bits(g, rg, S.DUALS_KEYS)
        S.same_bits(q, rq, S.RANGING_KEYS)
        A, b, c = at[:3]
        nonbasic = np.ones(n, bool)
        nonbasic[sol["basis"]] = False
        res[f"mixed_{m}x{n}"] = dict(
            shape=f"{m}x{n}", boxes=int(np.isfinite(at[4]).sum()), solve_iters=sol["iters"],
            duals_large=_stats(ms["duals_large"]), ranging_large=_stats(ms["ranging_large"]),
            plain_ranging=_stats(ms["plain_ranging"]),
            ranging_large_over_plain=round(float(np.median(ms["ranging_large"]) / np.median(ms["plain_ranging"])), 3),
            reference_one_core=dict(duals_ms=round(ref_d_ms, 1), ranging_ms=round(ref_r_ms, 1)),
            equal_to_the_reference_bit_for_bit=True,
            nonbasic_at_upper=int((at[6].astype(bool) & nonbasic).sum()), leaves_at_upper=int((q["b_side"] == 1).sum()),
            rel_w_minus_obj=float(abs(g["w"] - sol["obj"]) / max(1.0, abs(sol["obj"]))),
            values_in_their_ranges=bool(((q["b_lo"] <= b + 1e-9) & (b <= q["b_hi"] + 1e-9)).all() and
                                        ((q["c_lo"] <= c + 1e-9) & (c <= q["c_hi"] + 1e-9)).all()))
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
    main(args[0] if args else os.path.join(ROOT, "profiles", "bounded_sens_large.json"), "--calls-only" in sys.argv)
