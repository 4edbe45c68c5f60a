"""CPU-only checks of the batched two-phase C ABI: argument handling that needs no device."""
import ctypes as C

import numpy as np

from simplexmethod_amd import capi


def test_two_phase_batched_null_context():
    lib = capi.load()
    A = np.zeros(2 * 2 * 3)
    b, c = np.ones(2 * 2), np.ones(2 * 3)
    x, obj = np.zeros(2 * 3), np.zeros(2)
    bo, it, st = np.zeros(2 * 2, np.int32), np.zeros(2 * 3, np.int32), np.zeros(2, np.int32)
    rc = lib.lp_simplex_two_phase_batched(None, 2, capi._d(A), 2, 3, capi._d(b), capi._d(c), 0, 3, 1e-9, 100,
                                          capi._d(x), capi._i(bo), capi._d(obj), capi._i(it), capi._i(st))
    assert rc == capi.BAD_ARG
    h = C.c_void_p()
    rc = lib.lp_batched_two_phase_upload(None, 2, capi._d(A), 2, 3, capi._d(b), capi._d(c), 0, 3, C.byref(h))
    assert rc == capi.BAD_ARG and not h.value


def test_batched_path_and_phase_iters_reject_null():
    lib = capi.load()
    it = np.zeros(3, np.int32)
    assert lib.lp_batched_path(None) == capi.BAD_ARG
    assert lib.lp_batched_phase_iters(None, capi._i(it)) == capi.BAD_ARG
