"""Time of the Farkas / unbounded-ray certificates of bounded-variable LPs (lp_basis_bounded_certificate_batched) next
to the cold bounded solve that produced the bases (lp_simplex_bounded_batched) and to lp_basis_bounded_ranging_batched,
which does the same crash plus alpha work.
Workload: 4096 LPs of 32 x 96, seeds 0..4095, maximise, in turn tests/bounded_ref.boxed_lp "mixed" (mostly optimal),
"infeasible", "unbounded" and tests/bounded_certcases.rich_unbounded_lp, cold-solved; the certificates are computed at
the bases and flags the solve stopped at, once under its statuses (only the failed LPs are analysed) and once without
(every LP is).
Reports the median, min and max of 7 timed calls after one warm-up, host wall clock around the whole call (upload,
kernel, download).  The parts: `copies_and_launch` is the same call with every run status LP_OPTIMAL, so that every
workgroup leaves at once (upload + an empty launch + download); `kernel_by_difference` is the whole call minus that;
`upload` and `download` are one hipMemcpy each of the same numbers of bytes between pageable host memory and the
device.  The ranging entry refuses a basis with an artificial, so it runs on the LPs whose basis has none, and both
entries are also given per LP.
Checks the first 64 LPs against tests/ref/bounded_certificate_ref.c bit for bit and their vectors with numpy.
Writes profiles/bounded_certificate.json (or the path given as the first argument) and prints it.
With --calls-only it makes three calls of each entry and writes nothing: the workload for
`rocprofv3 --kernel-trace --stats -- python scripts/time_bounded_certificate.py --calls-only`, which gives the kernels'
own durations."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import bounded_certcases as BC  # noqa: E402
from tests import bounded_certificate_ref as R  # noqa: E402
from tests import bounded_ref as B  # noqa: E402

BATCH, REF_CHECKED, M, N = 4096, 64, 32, 96
KINDS = ("mixed", "infeasible", "unbounded", "rich")


def _timed(fn):
    fn()   # warm-up
    ms, out = [], None
    for _ in range(7):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def _hip_copies(up_bytes, down_bytes):
    """Median ms of one hipMemcpy of up_bytes host to device and one of down_bytes device to host (pageable host
    memory, the runtime the library itself uses), or (None, None) when the runtime cannot be reached."""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        return None, None
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    host = np.zeros(max(up_bytes, down_bytes), np.uint8)
    dev = C.c_void_p()
    if hip.hipSetDevice(0) != 0 or hip.hipMalloc(C.byref(dev), host.size) != 0:
        return None, None
    H2D, D2H = 1, 2

    def copy(dst, src, nbytes, kind):
        if hip.hipMemcpy(dst, src, nbytes, kind) != 0 or hip.hipDeviceSynchronize() != 0:
            raise RuntimeError("hipMemcpy failed")
    _, tu = _timed(lambda: copy(dev, host.ctypes.data, up_bytes, H2D))
    _, td = _timed(lambda: copy(host.ctypes.data, dev, down_bytes, D2H))
    hip.hipFree(dev)
    return tu, td


def main(path, calls_only=False):
    ctx = capi.Context(0)
    lps = [BC.rich_unbounded_lp(k, M, N, True) if KINDS[k % 4] == "rich" else
           B.boxed_lp(k, M, N, maximize=True, kind=KINDS[k % 4]) for k in range(BATCH)]
    A, b, c, lo, hi = (np.stack([lp[i] for lp in lps]) for i in range(5))
    if calls_only:
        cold = ctx.bounded_batched(A, b, c, lo, hi, True)
    else:
        cold, tc = _timed(lambda: ctx.bounded_batched(A, b, c, lo, hi, True))
    run = cold["status"]
    at = (A, b, c, lo, hi, cold["basis"], cold["at_upper"])
    real = np.flatnonzero((cold["basis"] < N).all(axis=1))   # no artificial: the ranging entry takes these
    at_real = tuple(v[real] for v in at)
    none_failed = np.zeros(BATCH, np.int32)
    if calls_only:
        for _ in range(3):
            ctx.basis_bounded_certificate_batched(*at, True, run_status=run)
            ctx.basis_bounded_certificate_batched(*at, True)
            ctx.bounded_ranging_batched(*at_real, True)
        ctx.close()
        return
    got, tf = _timed(lambda: ctx.basis_bounded_certificate_batched(*at, True, run_status=run))
    every, te = _timed(lambda: ctx.basis_bounded_certificate_batched(*at, True))
    _, t0 = _timed(lambda: ctx.basis_bounded_certificate_batched(*at, True, run_status=none_failed))
    on_real, tcr = _timed(lambda: ctx.basis_bounded_certificate_batched(*at_real, True))
    _, tr = _timed(lambda: ctx.bounded_ranging_batched(*at_real, True))
    want = R.certificate_batched(*(v[:REF_CHECKED] for v in at), True, run_status=run[:REF_CHECKED])
    R.same_bits({k: v[:REF_CHECKED] for k, v in got.items()}, want)
    want = R.certificate_batched(*(v[:REF_CHECKED] for v in at), True)
    R.same_bits({k: v[:REF_CHECKED] for k, v in every.items()}, want)
    for k in range(REF_CHECKED):
        BC.check(dict(A=A[k], b=b[k], c=c[k], lo=lo[k], hi=hi[k], maximize=True), {key: v[k] for key, v in every.items()})
    up_bytes = 8 * BATCH * (M * N + M + 3 * N) + 4 * BATCH * (M + N + 1)
    down_bytes = 8 * BATCH * (M + N + 1) + 4 * BATCH * 3
    tu, td = _hip_copies(up_bytes, down_bytes)
    failed = (run == 4) | (run == 1)
    res = dict(
        scenario=f"{BATCH} x {M}x{N}, maximise: boxed_lp mixed / infeasible / unbounded and rich_unbounded_lp in turn, "
                 "cold-solved by lp_simplex_bounded_batched, certificates at the bases and flags it stopped at; host "
                 "wall clock of the whole call, median of 7 after a warm-up",
        shape=f"{M}x{N}", lps=BATCH, run_optimal=int((run == 0).sum()), run_infeasible=int((run == 4).sum()),
        run_unbounded=int((run == 1).sum()), cold_solve=tc,
        certificate_failed_lps_only=tf, certificate_every_lp=te, copies_and_launch=t0,
        kernel_by_difference_failed_lps_only_ms=round(tf["ms_median"] - t0["ms_median"], 3),
        kernel_by_difference_every_lp_ms=round(te["ms_median"] - t0["ms_median"], 3),
        upload_bytes=up_bytes, download_bytes=down_bytes, upload=tu, download=td,
        lps_without_artificials=int(len(real)), certificate_on_those=tcr, ranging_on_those=tr,
        certificate_us_per_lp_on_those=round(1e3 * tcr["ms_median"] / len(real), 3),
        ranging_us_per_lp_on_those=round(1e3 * tr["ms_median"] / len(real), 3),
        farkas=int((got["kind"] == 1).sum()), rays=int((got["kind"] == 2).sum()),
        failed_without_certificate=int((failed & (got["kind"] == 0)).sum()),
        optimal_with_certificate=int(((run == 0) & (every["kind"] != 0)).sum()),
        certificate_statuses_on_those=sorted(set(on_real["status"].tolist())), ref_checked=REF_CHECKED)
    ctx.close()
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--calls-only"]
    main(args[0] if args else os.path.join(ROOT, "profiles", "bounded_certificate.json"), "--calls-only" in sys.argv)
