"""The bounded-variable simplex on a batch of boxed LPs (lp_simplex_bounded_batched) against the same LPs with the
boxes written as rows (lp_simplex_two_phase_batched).
Workloads, 4096 LPs each, seeds 0..4095, maximise:
  - boxed 32 x 96: tests/bounded_ref.boxed_lp(seed, 32, 96, kind="box"), every one of the 64 structural columns in
    [0, u]; its row form (bounded_ref.as_rows) is 96 x 160 and goes through lp_simplex_two_phase_batched;
  - boxed 64 x 192: the same generator; its row form (192 x 320) does not fit one CU's LDS, so only the bounded
    solve runs.
Reports the median, min and max of 7 timed calls after one warm-up (host wall clock around the whole call: upload,
kernel, download), the pivot and flip counts, the status histograms, and checks that both forms reach the same
objectives (1e-9 relative) and the first 64 bounded results against tests/ref/bounded_ref.c bit for bit.
Writes profiles/bounded.json (or the path given as the first argument) and prints it."""
import collections
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

BATCH, REF_CHECKED = 4096, 64
NAMES = {0: "optimal", 1: "unbounded", 2: "iter_limit", 3: "singular", 4: "infeasible", 5: "bad_arg"}


def _timed(fn):
    fn()   # warm-up
    ms, out = [], None
    for _ in range(7):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def _hist(status):
    return dict(sorted(collections.Counter(NAMES[int(s)] for s in status).items()))


def _batch(m, n):
    cases = [R.boxed_lp(k, m, n, maximize=True, kind="box") for k in range(BATCH)]
    return [np.stack([cs[i] for cs in cases]) for i in range(5)]


def main(path):
    ctx = capi.Context(0)
    res = {"scenario": f"{BATCH} x boxed_lp(seed, m, n, kind='box'): gen_lp with every structural column in [0, u], "
                       "maximise; host wall clock of the whole call, median of 7 after a warm-up"}
    for m, n in ((32, 96), (64, 192)):
        A, b, c, lo, hi = _batch(m, n)
        out, t = _timed(lambda: ctx.bounded_batched(A, b, c, lo, hi, True, n - m))
        it = out["iters"]
        for k in range(REF_CHECKED):
            r = R.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n - m)
            assert int(out["status"][k]) == r["status"] and [int(v) for v in it[k]] == r["iters"], k
            assert np.array_equal(out["basis"][k], r["basis"]) and (r["status"] or out["obj"][k] == r["obj"]), k
        entry = dict(t, shape=f"{m}x{n}", pivots_phase1=int(it[:, 0].sum()), pivots_driveout=int(it[:, 1].sum()),
                     pivots_phase2=int(it[:, 2].sum()), flips=int(it[:, 3].sum()), status=_hist(out["status"]),
                     fits=ctx.bounded_fits(m, n))
        rows = [R.as_rows(A[k], b[k], c[k], lo[k], hi[k]) for k in range(BATCH)]
        m2, n2 = rows[0][0].shape
        entry["row_form"] = f"{m2}x{n2}"
        if m == 32:
            A2 = np.stack([r[0] for r in rows])
            b2 = np.stack([r[1] for r in rows])
            c2 = np.stack([r[2] for r in rows])
            const = np.array([r[3] for r in rows])
            out2, t2 = _timed(lambda: ctx.two_phase_batched(A2, b2, c2, True, n2))
            ok = (out["status"] == 0) & (out2["status"] == 0)
            assert np.array_equal(out["status"], out2["status"])
            z2 = out2["obj"][ok] + const[ok]
            assert np.all(np.abs(out["obj"][ok] - z2) <= 1e-9 * np.maximum(1.0, np.abs(z2)))
            i2 = out2["iters"]
            entry["rows_two_phase"] = dict(t2, pivots_phase1=int(i2[:, 0].sum()), pivots_driveout=int(i2[:, 1].sum()),
                                           pivots_phase2=int(i2[:, 2].sum()), status=_hist(out2["status"]))
            entry["speedup_vs_rows"] = round(t2["ms_median"] / t["ms_median"], 2)
        res[f"boxed_{m}x{n}"] = entry
    ctx.close()
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bounded.json"))
