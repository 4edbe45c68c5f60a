"""Time of the dual solution and of RHS / cost ranging at bounded optima (lp_basis_bounded_duals_batched,
lp_basis_bounded_ranging_batched) next to the cold bounded solve that produced the bases (lp_simplex_bounded_batched).
Workloads, 4096 LPs each, seeds 0..4095, maximise: tests/bounded_ref.boxed_lp(seed, m, n) of 32 x 96 and 64 x 192,
cold-solved; the LPs that were optimal are analysed at their bases and flags.
Reports the median, min and max of 7 timed calls after one warm-up (host wall clock around the whole call: upload,
kernel, download) for the three entries, checks the first 64 LPs against tests/ref/bounded_sens_ref.c bit for bit, and
that w equals the solver's objective and every b_i and c_j lies in its own range.
Writes profiles/bounded_sens.json (or the path given as the first argument) and prints it.
With --calls-only it makes three calls of each entry per shape and writes nothing: the workload for
`rocprofv3 --kernel-trace --stats -- python scripts/time_bounded_sens.py --calls-only`, which gives the kernels' own
durations (the host wall clock is mostly the upload of A)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import bounded_ref as B  # noqa: E402
from tests import bounded_sens_ref as S  # noqa: E402

BATCH, REF_CHECKED = 4096, 64


def _timed(fn):
    fn()   # warm-up
    ms, out = [], None
    for _ in range(7):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def main(path, calls_only=False):
    ctx = capi.Context(0)
    res = {"scenario": f"{BATCH} x boxed_lp(seed, m, n), maximise, cold-solved by lp_simplex_bounded_batched; the optimal "
                       "ones analysed at their bases and flags by lp_basis_bounded_duals_batched and "
                       "lp_basis_bounded_ranging_batched; host wall clock of the whole call, median of 7 after a warm-up"}
    for m, n in ((32, 96), (64, 192)):
        cases = [B.boxed_lp(k, m, n, maximize=True) for k in range(BATCH)]
        A, b, c, lo, hi = (np.stack([cs[i] for cs in cases]) for i in range(5))
        if calls_only:
            first = ctx.bounded_batched(A, b, c, lo, hi, True)
        else:
            first, tc = _timed(lambda: ctx.bounded_batched(A, b, c, lo, hi, True))
        keep = np.flatnonzero(first["status"] == 0)
        at = (A[keep], b[keep], c[keep], lo[keep], hi[keep], first["basis"][keep], first["at_upper"][keep])
        if calls_only:
            for _ in range(3):
                ctx.bounded_duals_batched(*at)
                ctx.bounded_ranging_batched(*at, True)
            continue
        g, td = _timed(lambda: ctx.bounded_duals_batched(*at))
        q, tr = _timed(lambda: ctx.bounded_ranging_batched(*at, True))
        for k in range(REF_CHECKED):
            one = tuple(v[k] for v in at)
            S.same_bits({key: g[key][k] for key in S.DUALS_KEYS}, S.duals(*one), S.DUALS_KEYS)
            S.same_bits({key: q[key][k] for key in S.RANGING_KEYS}, S.ranging(*one, True), S.RANGING_KEYS)
        ok = (g["status"] == 0) & (q["status"] == 0)
        obj = first["obj"][keep]
        nb = np.ones(at[6].shape, bool)
        np.put_along_axis(nb, at[5].astype(np.int64), False, axis=1)
        res[f"boxed_{m}x{n}"] = dict(
            shape=f"{m}x{n}", lps=int(len(keep)), cold_solve_all_4096=tc, duals=td, ranging=tr,
            all_optimal=bool(ok.all()), nonbasic_at_upper=int((at[6].astype(bool) & nb).sum()),
            leaves_at_upper=int((q["b_side"] == 1).sum()),
            max_rel_w_minus_obj=float((np.abs(g["w"] - obj) / np.maximum(1.0, np.abs(obj)))[ok].max()),
            values_in_their_ranges=bool(((q["b_lo"] <= at[1] + 1e-9) & (at[1] <= q["b_hi"] + 1e-9))[ok].all() and
                                        ((q["c_lo"] <= at[2] + 1e-9) & (at[2] <= q["c_hi"] + 1e-9))[ok].all()),
            ref_checked=REF_CHECKED)
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
    main(args[0] if args else os.path.join(ROOT, "profiles", "bounded_sens.json"), "--calls-only" in sys.argv)
