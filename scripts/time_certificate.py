"""Time of the Farkas and ray certificates at the final bases (lp_batched_certificates) next to the solves that
produced them, and of the single-LP call (lp_basis_certificate) beyond lp_basis_certificate_fits.
  - 4096 LPs tests/certcases.two_phase_mix(0, 4096, 64, 128) (64 x 192: optimal, infeasible in one row, infeasible
    over several rows, unbounded in phase II, in turn): batched two-phase solve, then lp_batched_certificates;
  - 4096 LPs tests/certcases.plain_mix(0, 4096, 128, 256) (optimal, unbounded at the slack basis, unbounded after
    pivots): plain batched solve from the slack bases, then lp_batched_certificates (certificates for the unbounded
    LPs only) and lp_basis_certificate_batched at every final basis (all 4096 computed: the optimal ones run the
    full ray case and end NONE);
  - one LP certcases.unbounded_after_pivots(0, 512, 1024) at its final basis: lp_basis_certificate.
Each figure is the median (and spread) of 7 timed calls after one warm-up, host wall clock around the call (the
certificate calls include their device buffers and the copies of the vectors back to the host).
Writes profiles/certificate.json (or the path given as the first argument) and prints it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import certcases as CC  # noqa: E402


def timed(fn, runs=7):
    fn()   # warm-up
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def kinds(g):
    k = np.asarray(g["kind"])
    return {"none": int((k == capi.CERT_NONE).sum()), "farkas": int((k == capi.CERT_FARKAS).sum()),
            "ray": int((k == capi.CERT_RAY).sum())}


def batch_case(p):
    ms = [p.run() for _ in range(8)][1:]   # the kernel's own event time, warm-up dropped
    solve = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    s = p.download()
    g = p.certificates()
    st = s["status"]
    no_optimum = (st == capi.INFEASIBLE) | (st == capi.UNBOUNDED)
    return s, {"path": p.path(), "solve": solve, "certificates": timed(p.certificates),
               "run_status": {str(v): int((st == v).sum()) for v in np.unique(st)}, "kinds": kinds(g),
               "every_lp_without_optimum_certified": bool((np.asarray(g["kind"])[no_optimum] != 0).all())}


def main(path):
    ctx = capi.Context(0)
    res = {}
    A, b, c, _ = CC.two_phase_mix(0, 4096, 64, 128)
    p = ctx.batched_two_phase_problem(A, b, c, maximize=False)
    _, res["two_phase_4096x64x192"] = batch_case(p)
    p.free()
    A, b, c, B, _ = CC.plain_mix(0, 4096, 128, 256)
    p = ctx.batched_problem(A, b, c, B, True)
    s, res["plain_4096x128x256"] = batch_case(p)
    p.free()
    res["plain_4096x128x256"]["every_basis"] = timed(lambda: ctx.basis_certificate_batched(A, b, c, s["basis"], True))
    m, n = 512, 1024
    A, b, c, basis = CC.unbounded_after_pivots(0, m, n)
    q = ctx.simplex_problem(A, b, c, basis, True)
    rc, st = q.run()
    d = q.download()
    q.free()
    g = ctx.basis_certificate(A, b, c, d["basis"])
    res[f"single_{m}x{n}"] = {"fits": ctx.basis_certificate_fits(m, n), "run_status": int(rc),
                              "solve_ms": round(float(st.solve_ms), 4),
                              "certificate": timed(lambda: ctx.basis_certificate(A, b, c, d["basis"])),
                              "status": int(g["status"]), "kind": int(g["kind"])}
    ctx.close()
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "certificate.json"))
