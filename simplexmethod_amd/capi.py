"""ctypes binding of include/simplexmethod_amd.h (libsimplexmethod_hip.so).

There is no CPU fallback here or in the library: `load()` raises if the shared
object is missing, and `Context()` raises if no gfx950 device is usable.
Matrices are passed as (m, n) numpy arrays and converted to the ABI's column-major
layout (Eigen's default, /root/reference/src/ProblemTypes/Canonical.cpp:10).
"""
import collections
import ctypes as C
import os

import numpy as np

from . import build as _build

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
SUBSET_FEASIBLE, SUBSET_INFEASIBLE, SUBSET_SINGULAR = range(3)
SIMPLEX_AUTO, SIMPLEX_LAUNCH, SIMPLEX_LOOKAHEAD, SIMPLEX_RESIDENT, SIMPLEX_OVERLAP = 0, 1, 2, 3, 4
ENUM_AUTO, ENUM_DIRECT, ENUM_PREFIX = 0, 1, 2
PIVOT_DANTZIG, PIVOT_BLAND, PIVOT_DEVEX = 0, 1, 2
DUAL_DANTZIG, DUAL_DEVEX = 0, 1
DUAL_RATIO_TEXTBOOK, DUAL_RATIO_LONG_STEP = 0, 1
CERT_NONE, CERT_FARKAS, CERT_RAY = 0, 1, 2
U64_MAX = (1 << 64) - 1
EPS = 1e-9        # Solver::EPS, SimplexSolover.h:13
MAX_ITER = 10000  # SimplexSolover.h:426

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_u64p = C.POINTER(C.c_uint64)
_fp = C.POINTER(C.c_float)
_vp = C.c_void_p


class SimplexStats(C.Structure):
    _fields_ = [("status", C.c_int), ("pivots", C.c_int), ("launches", C.c_int),
                ("solve_ms", C.c_float), ("update_ms", C.c_float), ("update_launches", C.c_int),
                ("bytes_per_pivot", C.c_double), ("algo_used", C.c_int), ("fell_back", C.c_int)]


class EnumStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("subsets", C.c_uint64), ("launches", C.c_int)]


# name -> (restype, argtypes); also the list tests check against the header's declarations
SIGNATURES = {
    "lp_abi_version": (C.c_int, []),
    "lp_device_count": (C.c_int, []),
    "lp_context_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "lp_context_destroy": (None, [_vp]),
    "lp_last_error": (C.c_char_p, [_vp]),
    "lp_status_string": (C.c_char_p, [C.c_int]),
    "lp_context_sync": (C.c_int, [_vp]),
    "lp_simplex_solve": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int,
                                   C.c_double, C.c_int, _dp, _ip, _dp, _ip]),
    "lp_simplex_upload": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int,
                                    C.POINTER(_vp)]),
    "lp_simplex_solve_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int,
                                      C.c_double, C.c_int, _dp, _ip, _dp, _ip, C.c_int]),
    "lp_simplex_set_pivot_rule": (C.c_int, [_vp, C.c_int]),
    "lp_simplex_reset": (C.c_int, [_vp]),
    "lp_simplex_run": (C.c_int, [_vp, C.c_double, C.c_int, C.c_int, C.POINTER(SimplexStats)]),
    "lp_simplex_profile": (C.c_int, [_vp, C.c_int]),
    "lp_simplex_download": (C.c_int, [_vp, _dp, _ip, _dp, _ip, _ip, C.c_int, _dp]),
    "lp_simplex_free": (None, [_vp]),
    "lp_simplex_two_phase": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int,
                                       C.c_double, C.c_int, _dp, _ip, _dp, _ip]),
    "lp_simplex_two_phase_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int,
                                          C.c_double, C.c_int, _dp, _ip, _dp, _ip, C.c_int]),
    "lp_simplex_row": (C.c_int, [_vp, C.c_int, _dp]),
    "lp_simplex_force_pivot": (C.c_int, [_vp, C.c_int, C.c_int]),
    "lp_bench_rank1_update": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _fp]),
    "lp_bench_rankj_update": (C.c_int, [_vp, C.c_int, _fp, _ip]),
    "lp_debug_simplex_stamps": (C.c_int, [_vp, C.c_int, _u64p]),
    "lp_simplex_solve_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip,
                                           C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp,
                                           _ip, _ip]),
    "lp_simplex_solve_batched_ex": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip,
                                              C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp,
                                              _ip, _ip, C.c_int]),
    "lp_batched_set_pivot_rule": (C.c_int, [_vp, C.c_int]),
    "lp_batched_devex_fits": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "lp_batched_form": (C.c_int, [C.c_int, C.c_int, _ip]),
    "lp_batched_upload": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int,
                                    C.c_int, C.POINTER(_vp)]),
    "lp_batched_run": (C.c_int, [_vp, C.c_double, C.c_int, _fp]),
    "lp_batched_download": (C.c_int, [_vp, _dp, _ip, _dp, _ip, _ip]),
    "lp_batched_free": (None, [_vp]),
    "lp_batched_shard_bounds": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, _ip]),
    "lp_simplex_two_phase_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int,
                                               C.c_int, C.c_double, C.c_int, _dp, _ip, _dp, _ip, _ip]),
    "lp_simplex_two_phase_batched_ex": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int,
                                                  C.c_int, C.c_double, C.c_int, _dp, _ip, _dp, _ip, _ip,
                                                  C.c_int]),
    "lp_batched_two_phase_upload": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int,
                                              C.c_int, C.POINTER(_vp)]),
    "lp_batched_phase_iters": (C.c_int, [_vp, _ip]),
    "lp_batched_path": (C.c_int, [_vp]),
    "lp_simplex_resolve_run": (C.c_int, [_vp, C.c_double, C.c_int, _ip, C.POINTER(SimplexStats)]),
    "lp_simplex_resolve": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int, C.c_double,
                                     C.c_int, _dp, _ip, _dp, _ip]),
    "lp_simplex_resolve_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int,
                                             C.c_int, C.c_double, C.c_int, _dp, _ip, _dp, _ip, _ip]),
    "lp_batched_resolve_upload": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int,
                                            C.c_int, C.POINTER(_vp)]),
    "lp_batched_set_start": (C.c_int, [_vp, _dp, _ip]),
    "lp_batched_resolve_iters": (C.c_int, [_vp, _ip]),
    "lp_basis_duals": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _dp, _dp, _dp]),
    "lp_basis_duals_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _dp, _dp, _dp, _ip]),
    "lp_batched_duals": (C.c_int, [_vp, _dp, _dp, _dp, _ip]),
    "lp_basis_duals_fits": (C.c_int, [C.c_int]),
    "lp_basis_ranging": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_double, _dp, _ip, _dp,
                                   _ip]),
    "lp_basis_ranging_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_double,
                                           _dp, _ip, _dp, _ip, _ip]),
    "lp_batched_ranging": (C.c_int, [_vp, C.c_double, _dp, _ip, _dp, _ip, _ip]),
    "lp_basis_ranging_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_basis_certificate": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_double, _ip, _dp,
                                       _dp, _dp, _ip]),
    "lp_basis_certificate_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int,
                                               C.c_double, _ip, _dp, _dp, _dp, _ip, _ip]),
    "lp_batched_certificates": (C.c_int, [_vp, C.c_double, _ip, _dp, _dp, _dp, _ip, _ip]),
    "lp_basis_certificate_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_basis_parametric": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, _dp, C.c_double, C.c_double,
                                      C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip]),
    "lp_basis_parametric_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, _dp,
                                              C.c_double, C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip, _ip]),
    "lp_batched_parametric": (C.c_int, [_vp, _dp, C.c_double, C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip,
                                        _ip]),
    "lp_basis_parametric_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_basis_parametric_cost": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, _dp, C.c_double,
                                           C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip]),
    "lp_basis_parametric_cost_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, _dp,
                                                   C.c_double, C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip,
                                                   _ip]),
    "lp_batched_parametric_cost": (C.c_int, [_vp, _dp, C.c_double, C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip,
                                             _ip, _ip]),
    "lp_basis_parametric_cost_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_mip_solve": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int, _ip, C.c_double,
                               C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip]),
    "lp_mip_solve_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int, _ip,
                                       C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp,
                                       _ip, _ip, _ip]),
    "lp_batched_mip": (C.c_int, [_vp, _ip, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                 _dp, _ip, _ip, _ip]),
    "lp_mip_fits": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "lp_simplex_bounded": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double,
                                     C.c_int, _dp, _ip, _ip, _dp, _ip]),
    "lp_simplex_bounded_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int,
                                             C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, _ip]),
    "lp_simplex_bounded_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_simplex_bounded_large": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int,
                                           C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip]),
    "lp_simplex_bounded_resolve_large": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int,
                                             C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip]),
    "lp_simplex_bounded_resolve": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int,
                                             C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip]),
    "lp_simplex_bounded_resolve_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                                     C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip,
                                                     _ip]),
    "lp_simplex_bounded_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double,
                                        C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int]),
    "lp_simplex_bounded_batched_ex": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int,
                                                C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, _ip, C.c_int]),
    "lp_simplex_bounded_resolve_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int]),
    "lp_simplex_bounded_resolve_batched_ex": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip,
                                                        _ip, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp,
                                                        _ip, _ip, C.c_int]),
    "lp_simplex_bounded_rule_fits": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "lp_simplex_bounded_resolve_dual_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                     C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int,
                                                     C.c_int]),
    "lp_simplex_bounded_resolve_batched_dual_ex": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp,
                                                             _ip, _ip, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip,
                                                             _ip, _dp, _ip, _ip, C.c_int, C.c_int]),
    "lp_simplex_bounded_resolve_large_dual_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                                           C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp,
                                                           _ip, C.c_int, C.c_int]),
    "lp_simplex_bounded_dual_rule_fits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "lp_simplex_bounded_resolve_ratio_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                      C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int,
                                                      C.c_int, C.c_int]),
    "lp_simplex_bounded_resolve_batched_ratio_ex": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp,
                                                              _ip, _ip, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip,
                                                              _ip, _dp, _ip, _ip, C.c_int, C.c_int, C.c_int]),
    "lp_simplex_bounded_resolve_large_ratio_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                                            C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp,
                                                            _ip, C.c_int, C.c_int, C.c_int]),
    "lp_simplex_bounded_large_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int,
                                              C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int]),
    "lp_simplex_bounded_resolve_large_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                      C.c_int, C.c_double, C.c_int, _dp, _ip, _ip, _dp, _ip, C.c_int]),
    "lp_mip_bounded_solve": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int, _ip,
                                       C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp,
                                       _ip, _ip]),
    "lp_mip_bounded_solve_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, _ip,
                                               C.c_int, C.c_int, _ip, C.c_double, C.c_double, C.c_double, C.c_int,
                                               C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip, _ip]),
    "lp_mip_bounded_fits": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "lp_mip_bounded_solve_large": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int,
                                             _ip, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _dp,
                                             _dp, _dp, _ip, _ip]),
    "lp_mip_bounded_solve_large_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                C.c_int, _ip, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                                C.c_int, _dp, _dp, _dp, _ip, _ip, C.c_int]),
    "lp_mip_bounded_snapshot_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, _u64p]),
    "lp_mip_bounded_solve_ratio_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                C.c_int, _ip, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                                C.c_int, _dp, _dp, _dp, _ip, _ip, C.c_int]),
    "lp_mip_bounded_solve_batched_ratio_ex": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip,
                                                        _ip, _ip, C.c_int, C.c_int, _ip, C.c_double, C.c_double,
                                                        C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip,
                                                        _ip, C.c_int]),
    "lp_mip_bounded_solve_large_ratio_ex": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                      C.c_int, _ip, C.c_double, C.c_double, C.c_double, C.c_int,
                                                      C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip, C.c_int, C.c_int]),
    "lp_basis_bounded_duals": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _dp]),
    "lp_basis_bounded_duals_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                                 _dp, _dp, _dp, _dp, _ip]),
    "lp_basis_bounded_ranging": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                           C.c_double, _dp, _ip, _ip, _dp, _ip]),
    "lp_basis_bounded_ranging_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                                   C.c_int, C.c_double, _dp, _ip, _ip, _dp, _ip, _ip]),
    "lp_basis_bounded_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_basis_bounded_duals_large": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _dp, _dp,
                                               _dp]),
    "lp_basis_bounded_ranging_large": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                 C.c_double, _dp, _ip, _ip, _dp, _ip]),
    "lp_basis_bounded_certificate": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                               C.c_double, _ip, _dp, _dp, _dp, _ip]),
    "lp_basis_bounded_certificate_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip,
                                                       _ip, _ip, C.c_int, C.c_double, _ip, _dp, _dp, _dp, _ip, _ip]),
    "lp_basis_bounded_certificate_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_basis_bounded_certificate_large": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                     C.c_double, _ip, _dp, _dp, _dp, _ip]),
    "lp_basis_bounded_parametric": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, _dp,
                                              C.c_double, C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip, _ip,
                                              _ip]),
    "lp_basis_bounded_parametric_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip,
                                                      _ip, _ip, C.c_int, _dp, C.c_double, C.c_double, C.c_int, _ip,
                                                      _dp, _dp, _dp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "lp_basis_bounded_parametric_cost": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                   _dp, C.c_double, C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip,
                                                   _ip, _ip, _ip]),
    "lp_basis_bounded_parametric_cost_batched": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp,
                                                           _ip, _ip, _ip, C.c_int, _dp, C.c_double, C.c_double,
                                                           C.c_int, _ip, _dp, _dp, _dp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "lp_basis_bounded_parametric_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_basis_bounded_parametric_cost_fits": (C.c_int, [C.c_int, C.c_int]),
    "lp_basis_bounded_parametric_large": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int,
                                                    _dp, C.c_double, C.c_double, C.c_int, _ip, _dp, _dp, _dp, _ip, _ip,
                                                    _ip, _ip, _ip]),
    "lp_basis_bounded_parametric_cost_large": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                                         C.c_int, _dp, C.c_double, C.c_double, C.c_int, _ip, _dp, _dp,
                                                         _dp, _ip, _ip, _ip, _ip, _ip]),
    "lp_binom": (C.c_uint64, [C.c_int, C.c_int]),
    "lp_enum_shard_bounds": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _u64p, _u64p]),
    "lp_enum_solve": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _ip,
                                _u64p, _dp, _u64p]),
    "lp_enum_upload": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.POINTER(_vp)]),
    "lp_enum_range": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_int, _dp, _u64p,
                                C.POINTER(EnumStats)]),
    "lp_enum_first_within": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_double, C.c_double, _u64p]),
    "lp_enum_vertex": (C.c_int, [_vp, C.c_uint64, C.c_int, _dp, _ip, _dp, _ip]),
    "lp_enum_free": (None, [_vp]),
    "lp_enum_exact_division": (C.c_int, [_vp]),
    "lp_debug_reciprocal": (C.c_int, [_vp, _dp, C.c_int, _dp, _dp]),
    "lp_debug_division": (C.c_int, [_vp, _dp, _dp, C.c_int, _dp, _dp]),
    "lp_comm_unique_id": (C.c_int, [_vp]),
    "lp_comm_create_rccl": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    "lp_comm_create_local": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "lp_comm_rank": (C.c_int, [_vp]),
    "lp_comm_world": (C.c_int, [_vp]),
    "lp_comm_destroy": (None, [_vp]),
    "lp_enum_solve_sharded": (C.c_int, [_vp, _vp, C.c_int, _dp, _ip, _u64p, _dp, _u64p]),
    "lp_enum_shard_abstain": (C.c_int, [_vp, C.c_int]),
}

# phases of the chip-resident kernel's diagnostic instantiation (lp_debug_simplex_stamps after a
# chip-resident run: cycle sums per workgroup, in this order): slots 0-5 the communication wave
# (polls, decides, finishes the ratio test, publishes), slots 6-15 row wave 0
RESIDENT_STAMP_NAMES = [
    "comm: poll_records (the hop)", "comm: decide_and_decision_block",
    "comm: waits while the rows read the decision and stage the pivot row",
    "comm: waits for the rows' pricing + ratio slices, then ratio stage 2 + record",
    "comm: loop", "comm: commit",
    "rows: wait for the decision (publish -> hop -> decide)",
    "rows: read_decision_request_column_pivot_row_to_lds_two_quotients", "rows: pivot_row_barrier",
    "rows: reduced_costs_and_next_pricing", "rows: column_wait_eta_entry",
    "rows: candidate_ratio_slice", "rows: ratio_barrier",
    "rows: rank1_update_and_eta_column_publication", "rows: loop", "rows: commit"]

_lib = None


def lib_path():
    # LP_LIB_PATH: A/B experiments with an alternative build of the same library
    return os.environ.get("LP_LIB_PATH") or _build.HIP_LIB


def load():
    """Loads the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        if path == _build.HIP_LIB:   # a library older than its sources measures and tests something else
            srcs = [os.path.join(_build.CSRC, f) for f in os.listdir(_build.CSRC) if f.endswith((".hip", ".hpp"))]
            stale = [os.path.basename(f) for f in srcs if os.path.getmtime(f) > os.path.getmtime(path) + 1.0]
            if stale:
                import sys
                print(f"simplexmethod_amd: {os.path.basename(path)} is OLDER than {', '.join(sorted(stale))} - rebuild "
                      "(python -c 'import __graft_entry__ as g; g.build()')", file=sys.stderr)
        L = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError = ABI symbol missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def pivot_rule_id(rule):
    """"dantzig" | "bland" | "devex" | PIVOT_DANTZIG | PIVOT_BLAND | PIVOT_DEVEX -> the LP_PIVOT_* value (other
    integers pass through: the library refuses them with LP_BAD_ARG)."""
    if isinstance(rule, str):
        names = {"dantzig": PIVOT_DANTZIG, "bland": PIVOT_BLAND, "devex": PIVOT_DEVEX}
        if rule.lower() not in names:
            raise ValueError(f"unknown pivot rule {rule!r} (expected 'dantzig', 'bland' or 'devex')")
        return names[rule.lower()]
    return int(rule)


def dual_rule_id(rule):
    """"dantzig" | "devex" | DUAL_DANTZIG | DUAL_DEVEX -> the LP_DUAL_* value (other integers pass through: the
    library refuses them with LP_BAD_ARG)."""
    if isinstance(rule, str):
        names = {"dantzig": DUAL_DANTZIG, "devex": DUAL_DEVEX}
        if rule.lower() not in names:
            raise ValueError(f"unknown dual rule {rule!r} (expected 'dantzig' or 'devex')")
        return names[rule.lower()]
    return int(rule)


def dual_ratio_id(ratio):
    """"textbook" | "long_step" | DUAL_RATIO_TEXTBOOK | DUAL_RATIO_LONG_STEP -> the LP_DUAL_RATIO_* value (other
    integers pass through: the library refuses them with LP_BAD_ARG)."""
    if isinstance(ratio, str):
        names = {"textbook": DUAL_RATIO_TEXTBOOK, "long_step": DUAL_RATIO_LONG_STEP}
        if ratio.lower() not in names:
            raise ValueError(f"unknown dual ratio test {ratio!r} (expected 'textbook' or 'long_step')")
        return names[ratio.lower()]
    return int(ratio)


class LPError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"status {code}: {msg}")
        self.code = code


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def colmajor(A):
    A = np.asarray(A, dtype=np.float64)
    return np.ascontiguousarray(A.T).reshape(-1)


PackedLP = collections.namedtuple("PackedLP", "batch m n A b c basis lo hi at_upper")


def pack_lp(A, b, c, basis=None, lo=None, hi=None, at_upper=None, *, batched=False):
    """The ABI's form of an LP's arrays, or with `batched` of A (batch, m, n) and (batch, ...) vectors: a PackedLP
    with A column-major per LP and every array flat and contiguous, float64 (A, b, c, lo, hi) or int32 (basis,
    at_upper); what is not given stays None.  b and basis hold m entries per LP, the others n: anything else raises
    ValueError."""
    A = np.asarray(A, dtype=np.float64)
    batch, m, n = A.shape if batched else (1,) + A.shape
    Af = np.ascontiguousarray(np.transpose(A, (0, 2, 1))).reshape(-1) if batched else colmajor(A)
    out = []
    for name, v, dtype, per in (("b", b, np.float64, m), ("c", c, np.float64, n), ("basis", basis, np.int32, m),
                                ("lo", lo, np.float64, n), ("hi", hi, np.float64, n),
                                ("at_upper", at_upper, np.int32, n)):
        if v is not None:
            v = np.ascontiguousarray(v, dtype=dtype).reshape(-1)
            if v.size != batch * per:
                raise ValueError(f"{name}: expected {per} entries per LP ({batch * per}), got {v.size}")
        out.append(v)
    return PackedLP(batch, m, n, Af, *out)


# ---- synthetic LPs; bit-identical to oracle/lp_oracle.c:orc_gen_lp ----
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u01(key, count, start=0):
    with np.errstate(over="ignore"):
        k = np.arange(start + 1, start + count + 1, dtype=np.uint64)
        z = _mix64(np.uint64(key) + k * np.uint64(0x9E3779B97F4A7C15))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def gen_lp(seed, m, n):
    """Dense random canonical LP [A_orig | I]: A_orig ~ U(0,1), b ~ U(1,2)*(n-m)/2, c ~ U(0,1)
    on the original columns, slack basis, maximise.  Returns (A (m,n), b, c, basis)."""
    no = n - m
    with np.errstate(over="ignore"):
        key = int(_mix64(np.uint64(seed) + np.uint64(0x5851F42D4C957F2D)))
    u = _u01(key, no * m + m + no)
    A = np.zeros((m, n))
    A[:, :no] = u[:no * m].reshape(no, m).T
    A[:, no:] = np.eye(m)
    b = (1.0 + u[no * m:no * m + m]) * (no * 0.5)
    c = np.zeros(n)
    c[:no] = u[no * m + m:]
    basis = np.arange(no, n, dtype=np.int32)
    return A, b, c, basis


def batched_form(m, n):
    """lp_batched_form: the kernel form a plain m x n batch takes under Dantzig's rule, without a device.
    (fits, threads, rows_per_thread, aligned, dreg): fits says that the batch can run one LP per workgroup at all;
    threads = 0 is the LDS tableau, otherwise the register-resident kernel's workgroup size, row array and layout."""
    out = (C.c_int * 4)()
    fits = load().lp_batched_form(m, n, out)
    return (bool(fits), out[0], out[1], bool(out[2]), bool(out[3]))


MAX_BREAKS = 64  # default bound on the breakpoints of a parametric path
INT_TOL = 1e-6    # branch-and-bound defaults: integrality tolerance, pruning gap, depth and node limits
GAP = 1e-9
MAX_DEPTH = 32
MAX_NODES = 100000
MAX_DEPTH_BOUNDED = 64   # the bounded search keeps no tableau rows per level


def _mip_out(batch, n_orig, width=4):
    return (np.zeros((batch, n_orig)), np.zeros(batch), np.zeros(batch), np.zeros(batch, np.int32),
            np.zeros((batch, width), np.int32), np.zeros(batch, np.int32))


def _mip_dict(out):
    x, obj, bound, found, stats, st = out
    return dict(status=st, found=found, x=x, obj=obj, bound=bound, stats=stats)


def _mask(integer, n):
    integer = np.ascontiguousarray(integer, dtype=np.int32).reshape(-1)
    if integer.size != n:
        raise ValueError(f"integer mask: expected {n} entries, got {integer.size}")
    return integer


def _direction(v, size, what="the direction must have {size} entries, got {got}"):
    """The direction of a parametric call, flat float64; ValueError(`what`) unless it has `size` entries."""
    v = _f64(v).reshape(-1)
    if v.size != size:
        raise ValueError(what.format(size=size, got=v.size))
    return v


def _parametric_out(batch, m, max_breaks):
    """Zeroed output arrays of the batched parametric calls: nseg, t, obj, slope, enter, leave, basis, status."""
    mb = int(max_breaks)
    return (np.zeros(batch, np.int32), np.zeros((batch, mb + 2)), np.zeros((batch, mb + 2)),
            np.zeros((batch, mb + 1)), np.zeros((batch, mb + 1), np.int32), np.zeros((batch, mb + 1), np.int32),
            np.zeros((batch, m), np.int32), np.zeros(batch, np.int32))


def _parametric_dict(out):
    nseg, t, obj, slope, enter, leave, basis, st = out
    return dict(status=st, nseg=nseg, t=t, obj=obj, slope=slope, enter=enter, leave=leave, basis=basis)


def _ranging_dict(status, rhs, rhs_var, cost, cost_var):
    """Interleaved (lower, upper) pairs of the ranging calls -> dict(status, b_lo, b_hi, b_leave, c_lo, c_hi,
    c_enter); the last axis of b_leave / c_enter is (lower end, upper end)."""
    return dict(status=status, b_lo=rhs[..., 0::2], b_hi=rhs[..., 1::2],
                b_leave=rhs_var.reshape(rhs_var.shape[:-1] + (-1, 2)),
                c_lo=cost[..., 0::2], c_hi=cost[..., 1::2],
                c_enter=cost_var.reshape(cost_var.shape[:-1] + (-1, 2)))


class Context:
    """One HIP device + stream (lp_context)."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = _vp()
        rc = self.lib.lp_context_create(device, stream, C.byref(h))
        if rc != 0:
            raise LPError(rc, "lp_context_create failed: " +
                          (self.lib.lp_last_error(None) or b"").decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.lp_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self):
        return (self.lib.lp_last_error(self.h) or b"").decode()

    def check(self, rc):
        if rc < 0 or rc == BAD_ARG:
            raise LPError(rc, self.error() or self.lib.lp_status_string(rc).decode())
        return rc

    # ---- simplex -------------------------------------------------------------------------
    def debug_reciprocal(self, x):
        """(fast, plain): the leaf kernels' fast reciprocal of x and 1.0 / x, both from the device."""
        x = _f64(x).reshape(-1)
        fast, plain = np.empty_like(x), np.empty_like(x)
        self.check(self.lib.lp_debug_reciprocal(self.h, _d(x), len(x), _d(fast), _d(plain)))
        return fast, plain

    def debug_division(self, num, den):
        """(fast, plain): the chip-resident simplex's quotient sequence and num / den, both from the device."""
        num, den = _f64(num).reshape(-1), _f64(den).reshape(-1)
        fast, plain = np.empty_like(num), np.empty_like(num)
        self.check(self.lib.lp_debug_division(self.h, _d(num), _d(den), len(num), _d(fast), _d(plain)))
        return fast, plain

    def simplex_solve(self, A, b, c, basis, maximize=True, n_orig=None, eps=EPS,
                      max_iter=MAX_ITER, pivot_rule="dantzig"):
        p = pack_lp(A, b, c, basis)
        m, n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        n_orig = n if n_orig is None else n_orig
        x = np.zeros(max(n_orig, 1))
        bo = np.zeros(m, dtype=np.int32)
        obj = C.c_double(float("nan"))
        it = C.c_int(0)
        rc = self.check(self.lib.lp_simplex_solve_ex(self.h, _d(Af), m, n, _d(b), _d(c), _i(basis),
                                                     int(maximize), n_orig, eps, max_iter, _d(x),
                                                     _i(bo), C.byref(obj), C.byref(it),
                                                     pivot_rule_id(pivot_rule)))
        return dict(status=rc, x=x[:n_orig], basis=bo, obj=obj.value, iters=it.value)

    def two_phase(self, A, b, c, maximize=False, n_orig=None, eps=EPS, max_iter=MAX_ITER,
                  pivot_rule="dantzig"):
        """lp_simplex_two_phase: no starting basis needed."""
        p = pack_lp(A, b, c)
        m, n, Af, b, c = p.m, p.n, p.A, p.b, p.c
        n_orig = n if n_orig is None else n_orig
        x = np.zeros(n_orig)
        bo = np.full(m, -1, dtype=np.int32)
        obj = C.c_double(float("nan"))
        it = np.zeros(3, dtype=np.int32)
        rc = self.check(self.lib.lp_simplex_two_phase_ex(self.h, _d(Af), m, n, _d(b), _d(c),
                                                         int(maximize), n_orig, eps, max_iter, _d(x),
                                                         _i(bo), C.byref(obj), _i(it),
                                                         pivot_rule_id(pivot_rule)))
        return dict(status=rc, x=x, basis=bo, obj=obj.value, iters=it.tolist())

    def simplex_resolve(self, A, b, c, basis, maximize=True, n_orig=None, eps=EPS, max_iter=MAX_ITER):
        """lp_simplex_resolve: re-solve from `basis` (primal simplex if it is primal feasible, dual simplex if
        it is only dual feasible).  iters = (dual pivots, primal pivots).  A basis that is neither primal nor dual
        feasible raises LPError with code BAD_ARG."""
        p = pack_lp(A, b, c, basis)
        m, n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        n_orig = n if n_orig is None else n_orig
        x = np.zeros(max(n_orig, 1))
        bo = np.zeros(m, dtype=np.int32)
        obj = C.c_double(float("nan"))
        it = np.zeros(2, dtype=np.int32)
        rc = self.check(self.lib.lp_simplex_resolve(self.h, _d(Af), m, n, _d(b), _d(c), _i(basis), int(maximize),
                                                    n_orig, eps, max_iter, _d(x), _i(bo), C.byref(obj), _i(it)))
        return dict(status=rc, x=x[:n_orig], basis=bo, obj=obj.value, iters=(int(it[0]), int(it[1])))

    def resolve_batched(self, A, b, c, basis, maximize=True, n_orig=None, eps=EPS, max_iter=MAX_ITER):
        """lp_simplex_resolve_batched: A (batch, m, n), b (batch, m), c (batch, n), basis (batch, m); per LP
        exactly simplex_resolve().  iters: (batch, 2) = dual, primal pivots."""
        p = pack_lp(A, b, c, basis, batched=True)
        batch, m, n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        n_orig = n if n_orig is None else n_orig
        x = np.zeros((batch, n_orig))
        bo = np.zeros((batch, m), dtype=np.int32)
        obj = np.full(batch, np.nan)
        it = np.zeros((batch, 2), dtype=np.int32)
        st = np.zeros(batch, dtype=np.int32)
        self.check(self.lib.lp_simplex_resolve_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _i(basis),
                                                       int(maximize), n_orig, eps, max_iter, _d(x), _i(bo), _d(obj),
                                                       _i(it), _i(st)))
        return dict(status=st, x=x, basis=bo, obj=obj, iters=it)

    def batched_resolve_problem(self, A, b, c, basis, maximize=True, n_orig=None):
        """Device-resident re-solve batch (lp_batched_resolve_upload): set_start(), run(), download(),
        resolve_iters()."""
        return BatchedProblem(self, A, b, c, basis, maximize, n_orig, resolve=True)

    def simplex_problem(self, A, b, c, basis, maximize=True, n_orig=None):
        return SimplexProblem(self, A, b, c, basis, maximize, n_orig)

    # ---- the dual solution at a basis --------------------------------------------------------
    def basis_duals(self, A, b, c, basis):
        """lp_basis_duals: shadow prices y (m), reduced costs d (n) and w = b.y of the LP (A, b, c) at `basis`.
        dict(status, y, d, w); y, d, w are NaN unless status is OPTIMAL.  An index out of range raises LPError
        with code BAD_ARG."""
        p = pack_lp(A, b, c, basis)
        m, n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        y, d, w = np.zeros(m), np.zeros(n), C.c_double(0.0)
        rc = self.check(self.lib.lp_basis_duals(self.h, _d(Af), m, n, _d(b), _d(c), _i(basis), _d(y), _d(d),
                                                C.byref(w)))
        return dict(status=rc, y=y, d=d, w=w.value)

    def basis_duals_batched(self, A, b, c, basis):
        """lp_basis_duals_batched: A (batch, m, n), b (batch, m), c (batch, n), basis (batch, m).
        dict(status (batch), y (batch, m), d (batch, n), w (batch))."""
        p = pack_lp(A, b, c, basis, batched=True)
        batch, m, n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        y, d, w = np.zeros((batch, m)), np.zeros((batch, n)), np.zeros(batch)
        st = np.zeros(batch, dtype=np.int32)
        self.check(self.lib.lp_basis_duals_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _i(basis), _d(y),
                                                   _d(d), _d(w), _i(st)))
        return dict(status=st, y=y, d=d, w=w)

    def batched_devex_fits(self, m, n, two_phase=False):
        """lp_batched_devex_fits: True if the one-LP-per-workgroup kernel (plain or two-phase) holds an m x n LP
        together with its Devex weights."""
        return bool(self.lib.lp_batched_devex_fits(m, n, int(bool(two_phase))))

    def basis_duals_fits(self, m):
        """lp_basis_duals_fits: True if m runs the one-LP-per-workgroup kernel."""
        return bool(self.lib.lp_basis_duals_fits(m))

    # ---- RHS and cost ranging at a basis ------------------------------------------------------
    def basis_ranging(self, A, b, c, basis, maximize=True, eps=EPS):
        """lp_basis_ranging: how far each b_i and c_j can move before `basis` stops being feasible / optimal.
        dict(status, b_lo, b_hi (m), b_leave (m, 2), c_lo, c_hi (n), c_enter (n, 2)): the ends and the leaving /
        entering column at each (-1 for an infinite end); NaN and -1 unless status is OPTIMAL.  An index out of
        range or a negative eps raises LPError with code BAD_ARG."""
        p = pack_lp(A, b, c, basis)
        m, n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        rhs, cost = np.zeros(2 * m), np.zeros(2 * n)
        rv, cv = np.zeros(2 * m, np.int32), np.zeros(2 * n, np.int32)
        rc = self.check(self.lib.lp_basis_ranging(self.h, _d(Af), m, n, _d(b), _d(c), _i(basis), int(maximize),
                                                  float(eps), _d(rhs), _i(rv), _d(cost), _i(cv)))
        return _ranging_dict(rc, rhs, rv, cost, cv)

    def basis_ranging_batched(self, A, b, c, basis, maximize=True, eps=EPS):
        """lp_basis_ranging_batched: A (batch, m, n), b (batch, m), c (batch, n), basis (batch, m).  The dict of
        basis_ranging with a leading batch axis; status (batch)."""
        p = pack_lp(A, b, c, basis, batched=True)
        batch, m, n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        rhs, cost = np.zeros((batch, 2 * m)), np.zeros((batch, 2 * n))
        rv, cv = np.zeros((batch, 2 * m), np.int32), np.zeros((batch, 2 * n), np.int32)
        st = np.zeros(batch, dtype=np.int32)
        self.check(self.lib.lp_basis_ranging_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _i(basis),
                                                     int(maximize), float(eps), _d(rhs), _i(rv), _d(cost), _i(cv),
                                                     _i(st)))
        return _ranging_dict(st, rhs, rv, cost, cv)

    def basis_ranging_fits(self, m, n):
        """lp_basis_ranging_fits: True if an m x n LP runs the one-LP-per-workgroup kernel."""
        return bool(self.lib.lp_basis_ranging_fits(m, n))

    # ---- parametric right-hand side from an optimal basis --------------------------------------
    def basis_parametric(self, A, b, c, basis, d, t_max=np.inf, maximize=True, eps=EPS, max_breaks=MAX_BREAKS):
        """lp_basis_parametric: the optimal value along b + t d for t in [0, t_max] from the optimal `basis`.
        dict(status, t (nseg+1), obj (nseg+1), slope (nseg), enter (nseg), leave (nseg), basis (m)): breakpoints,
        the optimal value at each, the slope of each segment and the pivot that ends it (enter -1 on the last one).
        status OPTIMAL (reached t_max), INFEASIBLE (infeasible past t[-1]), ITER_LIMIT (max_breaks pivots done) or
        SINGULAR (empty arrays).  A basis that is not optimal at t = 0, an index out of range, t_max < 0, eps < 0 or
        max_breaks < 0 raises LPError with code BAD_ARG."""
        p = pack_lp(A, b, c, basis)
        m, n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        d = _direction(d, m)
        out = _parametric_out(1, m, max(int(max_breaks), 0))
        nseg, t, obj, slope, enter, leave, bo, _ = out
        rc = self.check(self.lib.lp_basis_parametric(self.h, _d(Af), m, n, _d(b), _d(c), _i(basis), int(maximize),
                                                     _d(d), float(t_max), float(eps), int(max_breaks), _i(nseg),
                                                     _d(t), _d(obj), _d(slope), _i(enter), _i(leave), _i(bo)))
        ns = int(nseg[0])
        return dict(status=rc, t=t[0, :ns + 1] if ns else t[0, :0], obj=obj[0, :ns + 1] if ns else obj[0, :0],
                    slope=slope[0, :ns], enter=enter[0, :ns], leave=leave[0, :ns], basis=bo[0])

    def basis_parametric_batched(self, A, b, c, basis, d, t_max=np.inf, maximize=True, eps=EPS,
                                 max_breaks=MAX_BREAKS):
        """lp_basis_parametric_batched: A (batch, m, n), b (batch, m), c (batch, n), basis (batch, m), d (batch, m).
        dict(status (batch), nseg (batch), t, obj (batch, max_breaks+2), slope, enter, leave (batch, max_breaks+1),
        basis (batch, m)), padded with NaN / -1 past each path."""
        p = pack_lp(A, b, c, basis, batched=True)
        batch, m, n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        d = _direction(d, batch * m)
        out = _parametric_out(batch, m, max(int(max_breaks), 0))
        nseg, t, obj, slope, enter, leave, bo, st = out
        self.check(self.lib.lp_basis_parametric_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _i(basis),
                                                        int(maximize), _d(d), float(t_max), float(eps),
                                                        int(max_breaks), _i(nseg), _d(t), _d(obj), _d(slope),
                                                        _i(enter), _i(leave), _i(bo), _i(st)))
        return _parametric_dict(out)

    def basis_parametric_fits(self, m, n):
        """lp_basis_parametric_fits: True if an m x n LP runs the one-LP-per-workgroup kernel."""
        return bool(self.lib.lp_basis_parametric_fits(m, n))

    # ---- parametric cost from an optimal basis -------------------------------------------------
    def basis_parametric_cost(self, A, b, c, basis, g, t_max=np.inf, maximize=True, eps=EPS, max_breaks=MAX_BREAKS):
        """lp_basis_parametric_cost: the optimal value along c + t g for t in [0, t_max] from the optimal `basis`.
        dict(status, t (nseg+1), obj (nseg+1), slope (nseg), enter (nseg), leave (nseg), basis (m)): breakpoints,
        the optimal value at each, the slope of each segment and the pivot that ends it (leave -1 on the last one).
        status OPTIMAL (reached t_max), UNBOUNDED (unbounded past t[-1]), ITER_LIMIT (max_breaks pivots done) or
        SINGULAR (empty arrays).  A basis that is not optimal at t = 0, an index out of range, t_max < 0, eps < 0 or
        max_breaks < 0 raises LPError with code BAD_ARG."""
        p = pack_lp(A, b, c, basis)
        m, n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        g = _direction(g, n)
        out = _parametric_out(1, m, max(int(max_breaks), 0))
        nseg, t, obj, slope, enter, leave, bo, _ = out
        rc = self.check(self.lib.lp_basis_parametric_cost(self.h, _d(Af), m, n, _d(b), _d(c), _i(basis),
                                                          int(maximize), _d(g), float(t_max), float(eps),
                                                          int(max_breaks), _i(nseg), _d(t), _d(obj), _d(slope),
                                                          _i(enter), _i(leave), _i(bo)))
        ns = int(nseg[0])
        return dict(status=rc, t=t[0, :ns + 1] if ns else t[0, :0], obj=obj[0, :ns + 1] if ns else obj[0, :0],
                    slope=slope[0, :ns], enter=enter[0, :ns], leave=leave[0, :ns], basis=bo[0])

    def basis_parametric_cost_batched(self, A, b, c, basis, g, t_max=np.inf, maximize=True, eps=EPS,
                                      max_breaks=MAX_BREAKS):
        """lp_basis_parametric_cost_batched: A (batch, m, n), b (batch, m), c (batch, n), basis (batch, m),
        g (batch, n).  dict(status (batch), nseg (batch), t, obj (batch, max_breaks+2), slope, enter, leave
        (batch, max_breaks+1), basis (batch, m)), padded with NaN / -1 past each path."""
        p = pack_lp(A, b, c, basis, batched=True)
        batch, m, n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        g = _direction(g, batch * n)
        out = _parametric_out(batch, m, max(int(max_breaks), 0))
        nseg, t, obj, slope, enter, leave, bo, st = out
        self.check(self.lib.lp_basis_parametric_cost_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _i(basis),
                                                             int(maximize), _d(g), float(t_max), float(eps),
                                                             int(max_breaks), _i(nseg), _d(t), _d(obj), _d(slope),
                                                             _i(enter), _i(leave), _i(bo), _i(st)))
        return _parametric_dict(out)

    def basis_parametric_cost_fits(self, m, n):
        """lp_basis_parametric_cost_fits: True if an m x n LP runs the one-LP-per-workgroup kernel."""
        return bool(self.lib.lp_basis_parametric_cost_fits(m, n))

    # ---- depth-first branch-and-bound for integer LPs -------------------------------------------
    def mip(self, A, b, c, basis, integer, maximize=True, n_orig=None, eps=EPS, int_tol=INT_TOL, gap=GAP,
            max_depth=MAX_DEPTH, max_nodes=MAX_NODES, max_iter=MAX_ITER):
        """lp_mip_solve: opt c.x, A x = b, x >= 0, x_j integral where integer[j] (n entries, 0/1, j < n_orig), from
        the root basis `basis` (as resolve: primal or dual feasible).  dict(status, found, x (n_orig), obj, bound,
        stats (nodes, dual pivots, primal pivots, deepest level)); x and obj NaN without an incumbent.  A basis that
        is no valid start, a bad argument or a shape beyond mip_fits raises LPError with code BAD_ARG."""
        p = pack_lp(A, b, c, basis)
        m, n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        n_orig = n if n_orig is None else int(n_orig)
        integer = _mask(integer, n)
        x, obj, bound, found, stats, _ = _mip_out(1, n_orig)
        rc = self.check(self.lib.lp_mip_solve(self.h, _d(Af), m, n, _d(b), _d(c), _i(basis), int(maximize), n_orig,
                                              _i(integer), float(eps), float(int_tol), float(gap), int(max_depth),
                                              int(max_nodes), int(max_iter), _d(x), _d(obj), _d(bound), _i(found),
                                              _i(stats)))
        return dict(status=rc, found=int(found[0]), x=x[0], obj=float(obj[0]), bound=float(bound[0]),
                    stats=tuple(int(v) for v in stats[0]))

    def mip_batched(self, A, b, c, basis, integer, maximize=True, n_orig=None, eps=EPS, int_tol=INT_TOL, gap=GAP,
                    max_depth=MAX_DEPTH, max_nodes=MAX_NODES, max_iter=MAX_ITER):
        """lp_mip_solve_batched: A (batch, m, n), b (batch, m), c (batch, n), basis (batch, m), one mask (n).
        dict(status, found, obj, bound (batch), x (batch, n_orig), stats (batch, 4))."""
        p = pack_lp(A, b, c, basis, batched=True)
        batch, m, n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        n_orig = n if n_orig is None else int(n_orig)
        integer = _mask(integer, n)
        out = _mip_out(batch, n_orig)
        x, obj, bound, found, stats, st = out
        self.check(self.lib.lp_mip_solve_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _i(basis), int(maximize),
                                                 n_orig, _i(integer), float(eps), float(int_tol), float(gap),
                                                 int(max_depth), int(max_nodes), int(max_iter), _d(x), _d(obj),
                                                 _d(bound), _i(found), _i(stats), _i(st)))
        return _mip_dict(out)

    def mip_fits(self, m, n, max_depth=MAX_DEPTH):
        """lp_mip_fits: True if an m x n problem searched to max_depth fits one CU's LDS."""
        return bool(self.lib.lp_mip_fits(m, n, max_depth))

    # ---- bounded-variable simplex -------------------------------------------------------------
    dual_rule_id = staticmethod(dual_rule_id)
    dual_ratio_id = staticmethod(dual_ratio_id)

    def _bounded_call(self, name, pivot_rule, *args, dual_rule=None, dual_ratio=None):
        """The entry `name` of the bounded family, or with a pivot_rule its _ex form with the rule appended, or (the
        re-solves) with a dual_rule its _dual_ex form with both appended (no pivot_rule: Dantzig's), or with a
        dual_ratio its _ratio_ex form with all three appended (no dual_rule: Dantzig's)."""
        if dual_ratio is not None:
            rule = PIVOT_DANTZIG if pivot_rule is None else pivot_rule_id(pivot_rule)
            dual = DUAL_DANTZIG if dual_rule is None else dual_rule_id(dual_rule)
            return self.check(getattr(self.lib, name + "_ratio_ex")(*args, rule, dual, dual_ratio_id(dual_ratio)))
        if dual_rule is not None:
            rule = PIVOT_DANTZIG if pivot_rule is None else pivot_rule_id(pivot_rule)
            return self.check(getattr(self.lib, name + "_dual_ex")(*args, rule, dual_rule_id(dual_rule)))
        if pivot_rule is None:
            return self.check(getattr(self.lib, name)(*args))
        return self.check(getattr(self.lib, name + "_ex")(*args, pivot_rule_id(pivot_rule)))

    def bounded(self, A, b, c, lo, hi, maximize=False, n_orig=None, eps=EPS, max_iter=MAX_ITER, pivot_rule=None):
        """lp_simplex_bounded: opt c.x, A x = b, lo <= x <= hi (lo finite, hi finite or inf), no starting basis.
        pivot_rule ("dantzig", "bland", "devex" or a PIVOT_* value; None: the entry without a rule, which is Dantzig's)
        goes through lp_simplex_bounded_ex and holds in both phases; an unknown rule or, under Devex, a shape beyond
        bounded_rule_fits raises LPError with code BAD_ARG.
        dict(status, x (n_orig), basis (m), at_upper (n, 0/1), obj, iters (phase-I pivots, drive-out pivots, phase-II
        pivots, bound flips)); x NaN and obj NaN unless OPTIMAL.  A bad bound or a shape beyond bounded_fits raises
        LPError with code BAD_ARG."""
        p = pack_lp(A, b, c, lo=lo, hi=hi)
        m, n, Af, b, c, lo, hi = p.m, p.n, p.A, p.b, p.c, p.lo, p.hi
        n_orig = n if n_orig is None else int(n_orig)
        x = np.full(n_orig, np.nan)
        bo = np.full(m, -1, dtype=np.int32)
        up = np.zeros(n, dtype=np.int32)
        obj = np.full(1, np.nan)
        it = np.zeros(4, dtype=np.int32)
        rc = self._bounded_call("lp_simplex_bounded", pivot_rule, self.h, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi),
                                int(maximize), n_orig, float(eps), int(max_iter), _d(x), _i(bo), _i(up), _d(obj), _i(it))
        return dict(status=rc, x=x, basis=bo, at_upper=up, obj=float(obj[0]), iters=it.tolist())

    def bounded_batched(self, A, b, c, lo, hi, maximize=False, n_orig=None, eps=EPS, max_iter=MAX_ITER,
                        pivot_rule=None):
        """lp_simplex_bounded_batched: A (batch, m, n), b (batch, m), c / lo / hi (batch, n).  dict(status (batch),
        x (batch, n_orig), basis (batch, m), at_upper (batch, n), obj (batch), iters (batch, 4)); per LP exactly
        bounded(), pivot_rule included (lp_simplex_bounded_batched_ex)."""
        p = pack_lp(A, b, c, lo=lo, hi=hi, batched=True)
        batch, m, n, Af, b, c, lo, hi = p.batch, p.m, p.n, p.A, p.b, p.c, p.lo, p.hi
        n_orig = n if n_orig is None else int(n_orig)
        x = np.full((batch, n_orig), np.nan)
        bo = np.full((batch, m), -1, dtype=np.int32)
        up = np.zeros((batch, n), dtype=np.int32)
        obj = np.full(batch, np.nan)
        it = np.zeros((batch, 4), dtype=np.int32)
        st = np.zeros(batch, dtype=np.int32)
        self._bounded_call("lp_simplex_bounded_batched", pivot_rule, self.h, batch, _d(Af), m, n, _d(b), _d(c), _d(lo),
                           _d(hi), int(maximize), n_orig, float(eps), int(max_iter), _d(x), _i(bo), _i(up), _d(obj),
                           _i(it), _i(st))
        return dict(status=st, x=x, basis=bo, at_upper=up, obj=obj, iters=it)

    def bounded_large(self, A, b, c, lo, hi, maximize=False, n_orig=None, eps=EPS, max_iter=MAX_ITER,
                      pivot_rule=None):
        """lp_simplex_bounded_large: the LP of bounded() on the tableau in HBM, at any shape two_phase() runs (no
        bounded_fits limit).  pivot_rule as in bounded() (None: the entry without a rule, which is Dantzig's; else
        lp_simplex_bounded_large_ex, no bounded_rule_fits limit either).  Returns the dict of bounded(), equal to it
        under the same rule where both run."""
        p = pack_lp(A, b, c, lo=lo, hi=hi)
        m, n, Af, b, c, lo, hi = p.m, p.n, p.A, p.b, p.c, p.lo, p.hi
        n_orig = n if n_orig is None else int(n_orig)
        x = np.full(n_orig, np.nan)
        bo = np.full(m, -1, dtype=np.int32)
        up = np.zeros(n, dtype=np.int32)
        obj = np.full(1, np.nan)
        it = np.zeros(4, dtype=np.int32)
        rc = self._bounded_call("lp_simplex_bounded_large", pivot_rule, self.h, _d(Af), m, n, _d(b), _d(c), _d(lo),
                                _d(hi), int(maximize), n_orig, float(eps), int(max_iter), _d(x), _i(bo), _i(up),
                                _d(obj), _i(it))
        return dict(status=rc, x=x, basis=bo, at_upper=up, obj=float(obj[0]), iters=it.tolist())

    def bounded_resolve_large(self, A, b, c, lo, hi, basis, at_upper, maximize=False, n_orig=None, eps=EPS,
                              max_iter=MAX_ITER, pivot_rule=None, dual_rule=None, dual_ratio=None):
        """lp_simplex_bounded_resolve_large: the re-solve of bounded_resolve() on the tableau in HBM, at any shape
        bounded_large() runs (no bounded_fits limit).  pivot_rule as in bounded_resolve() (None: the entry without a
        rule; else lp_simplex_bounded_resolve_large_ex): it governs the primal loop only.  Returns the dict of
        bounded_resolve(), equal to it under the same rules where both run; refusals as there.  dual_rule as in
        bounded_resolve() (lp_simplex_bounded_resolve_large_dual_ex; the m weights live in device memory, no
        bounded_dual_rule_fits limit), dual_ratio as there (lp_simplex_bounded_resolve_large_ratio_ex)."""
        p = pack_lp(A, b, c, basis, lo, hi, at_upper)
        m, n, Af, b, c, basis, lo, hi, at_upper = p.m, p.n, p.A, p.b, p.c, p.basis, p.lo, p.hi, p.at_upper
        n_orig = n if n_orig is None else int(n_orig)
        x = np.full(n_orig, np.nan)
        bo = np.full(m, -1, dtype=np.int32)
        up = np.zeros(n, dtype=np.int32)
        obj = np.full(1, np.nan)
        it = np.zeros(3, dtype=np.int32)
        rc = self._bounded_call("lp_simplex_bounded_resolve_large", pivot_rule, self.h, _d(Af), m, n, _d(b), _d(c),
                                _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize), n_orig, float(eps),
                                int(max_iter), _d(x), _i(bo), _i(up), _d(obj), _i(it), dual_rule=dual_rule, dual_ratio=dual_ratio)
        return dict(status=rc, x=x, basis=bo, at_upper=up, obj=float(obj[0]), iters=it.tolist())

    def bounded_fits(self, m, n):
        """lp_simplex_bounded_fits: True if an m x n bounded LP fits one CU's LDS."""
        return bool(self.lib.lp_simplex_bounded_fits(m, n))

    def bounded_rule_fits(self, m, n, pivot_rule):
        """lp_simplex_bounded_rule_fits: True if an m x n bounded LP fits one CU's LDS under pivot_rule: bounded_fits,
        and under PIVOT_DEVEX with n more doubles, the weights.  False for an unknown rule."""
        return bool(self.lib.lp_simplex_bounded_rule_fits(m, n, pivot_rule_id(pivot_rule)))

    def bounded_dual_rule_fits(self, m, n, pivot_rule, dual_rule):
        """lp_simplex_bounded_dual_rule_fits: True if an m x n bounded re-solve fits one CU's LDS under both rules:
        bounded_fits plus the larger of n doubles (PIVOT_DEVEX) and m doubles (DUAL_DEVEX), one region for the loop
        that runs.  False for an unknown rule of either kind."""
        return bool(self.lib.lp_simplex_bounded_dual_rule_fits(m, n, pivot_rule_id(pivot_rule), dual_rule_id(dual_rule)))

    def bounded_resolve(self, A, b, c, lo, hi, basis, at_upper, maximize=False, n_orig=None, eps=EPS,
                        max_iter=MAX_ITER, pivot_rule=None, dual_rule=None, dual_ratio=None):
        """lp_simplex_bounded_resolve: the LP of bounded() re-solved from `basis` (m) and `at_upper` (n, 0/1), normally
        an earlier result's, after a change of lo, hi, b or c: the bounded primal loop if the basis is primal feasible,
        the bounded dual simplex if it is only dual feasible.  dict as bounded() with iters = (dual pivots, primal
        pivots, bound flips).  A basis that is neither, a bad index or flag, a bad bound or a shape beyond bounded_fits
        raises LPError with code BAD_ARG.  pivot_rule as in bounded() (lp_simplex_bounded_resolve_ex): it governs the
        primal loop only; the dual simplex is the same under every pivot rule.  dual_rule ("dantzig", "devex" or a
        DUAL_* value; None: the call made without it) goes through lp_simplex_bounded_resolve_dual_ex and governs the
        leaving choice of the dual simplex only: under "devex" status and objective are Dantzig's up to rounding, the
        optimal basis and the pivot count may differ.  An unknown dual rule or a shape beyond bounded_dual_rule_fits
        raises LPError with code BAD_ARG.  dual_ratio ("textbook", "long_step" or a DUAL_RATIO_* value; None: the call
        made without it) goes through lp_simplex_bounded_resolve_ratio_ex and governs the entering step of the dual
        simplex only: under "long_step" (the bound-flipping ratio test) a candidate whose flip to its other bound leaves
        the leaving row violated is flipped, not pivoted on, and iters[2] counts those flips; status and objective are
        the textbook test's up to rounding.  An unknown dual ratio raises LPError with code BAD_ARG."""
        p = pack_lp(A, b, c, basis, lo, hi, at_upper)
        m, n, Af, b, c, basis, lo, hi, at_upper = p.m, p.n, p.A, p.b, p.c, p.basis, p.lo, p.hi, p.at_upper
        n_orig = n if n_orig is None else int(n_orig)
        x = np.full(n_orig, np.nan)
        bo = np.full(m, -1, dtype=np.int32)
        up = np.zeros(n, dtype=np.int32)
        obj = np.full(1, np.nan)
        it = np.zeros(3, dtype=np.int32)
        rc = self._bounded_call("lp_simplex_bounded_resolve", pivot_rule, self.h, _d(Af), m, n, _d(b), _d(c), _d(lo),
                                _d(hi), _i(basis), _i(at_upper), int(maximize), n_orig, float(eps), int(max_iter), _d(x),
                                _i(bo), _i(up), _d(obj), _i(it), dual_rule=dual_rule, dual_ratio=dual_ratio)
        return dict(status=rc, x=x, basis=bo, at_upper=up, obj=float(obj[0]), iters=it.tolist())

    def bounded_resolve_batched(self, A, b, c, lo, hi, basis, at_upper, maximize=False, n_orig=None, eps=EPS,
                                max_iter=MAX_ITER, pivot_rule=None, dual_rule=None, dual_ratio=None):
        """lp_simplex_bounded_resolve_batched: arrays as bounded_batched(), basis (batch, m), at_upper (batch, n).
        dict as bounded_batched() with iters (batch, 3); per LP exactly bounded_resolve(), except that a basis that
        is no valid start is that LP's status BAD_ARG.  pivot_rule as in bounded_resolve()
        (lp_simplex_bounded_resolve_batched_ex), dual_rule as there (lp_simplex_bounded_resolve_batched_dual_ex),
        dual_ratio as there (lp_simplex_bounded_resolve_batched_ratio_ex)."""
        p = pack_lp(A, b, c, basis, lo, hi, at_upper, batched=True)
        batch, m, n, Af, b, c = p.batch, p.m, p.n, p.A, p.b, p.c
        basis, lo, hi, at_upper = p.basis, p.lo, p.hi, p.at_upper
        n_orig = n if n_orig is None else int(n_orig)
        x = np.full((batch, n_orig), np.nan)
        bo = np.full((batch, m), -1, dtype=np.int32)
        up = np.zeros((batch, n), dtype=np.int32)
        obj = np.full(batch, np.nan)
        it = np.zeros((batch, 3), dtype=np.int32)
        st = np.zeros(batch, dtype=np.int32)
        self._bounded_call("lp_simplex_bounded_resolve_batched", pivot_rule, self.h, batch, _d(Af), m, n, _d(b), _d(c),
                           _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize), n_orig, float(eps), int(max_iter),
                           _d(x), _i(bo), _i(up), _d(obj), _i(it), _i(st), dual_rule=dual_rule, dual_ratio=dual_ratio)
        return dict(status=st, x=x, basis=bo, at_upper=up, obj=obj, iters=it)

    # ---- the dual solution and ranging of a bounded-variable LP at a basis ----------------------
    def bounded_duals(self, A, b, c, lo, hi, basis, at_upper):
        """lp_basis_bounded_duals: the LP of bounded() at `basis` (m) and `at_upper` (n, 0/1), normally a result's: the
        point x (n) they define, shadow prices y (m), reduced costs d (n) and w = b.y + sum d_j x_j over the non-basic
        columns (c.x at an optimum), in the original variables.  dict(status, x, y, d, w); NaN unless status is
        OPTIMAL (SINGULAR: a crash failed; INFEASIBLE: some hi < lo).  A bad bound, index or flag or a shape beyond
        basis_bounded_fits raises LPError with code BAD_ARG."""
        return self._bounded_duals(self.lib.lp_basis_bounded_duals, A, b, c, lo, hi, basis, at_upper)

    def bounded_duals_large(self, A, b, c, lo, hi, basis, at_upper):
        """lp_basis_bounded_duals_large: bounded_duals() on the tableau in HBM, at any shape bounded_large() runs (no
        basis_bounded_fits limit).  Returns the dict of bounded_duals(), equal to it where both run; refusals as there."""
        return self._bounded_duals(self.lib.lp_basis_bounded_duals_large, A, b, c, lo, hi, basis, at_upper)

    def _bounded_duals(self, entry, A, b, c, lo, hi, basis, at_upper):
        p = pack_lp(A, b, c, basis, lo, hi, at_upper)
        m, n, Af, b, c, basis, lo, hi, at_upper = p.m, p.n, p.A, p.b, p.c, p.basis, p.lo, p.hi, p.at_upper
        x, y, d, w = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(1)
        rc = self.check(entry(self.h, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), _d(x),
                              _d(y), _d(d), _d(w)))
        return dict(status=rc, x=x, y=y, d=d, w=float(w[0]))

    def bounded_duals_batched(self, A, b, c, lo, hi, basis, at_upper):
        """lp_basis_bounded_duals_batched: A (batch, m, n), b (batch, m), c / lo / hi / at_upper (batch, n), basis
        (batch, m).  The dict of bounded_duals with a leading batch axis; status (batch)."""
        p = pack_lp(A, b, c, basis, lo, hi, at_upper, batched=True)
        batch, m, n, Af, b, c = p.batch, p.m, p.n, p.A, p.b, p.c
        basis, lo, hi, at_upper = p.basis, p.lo, p.hi, p.at_upper
        x, y, d, w = np.zeros((batch, n)), np.zeros((batch, m)), np.zeros((batch, n)), np.zeros(batch)
        st = np.zeros(batch, dtype=np.int32)
        self.check(self.lib.lp_basis_bounded_duals_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi),
                                                           _i(basis), _i(at_upper), _d(x), _d(y), _d(d), _d(w), _i(st)))
        return dict(status=st, x=x, y=y, d=d, w=w)

    def bounded_ranging(self, A, b, c, lo, hi, basis, at_upper, maximize=False, eps=EPS):
        """lp_basis_bounded_ranging: how far each b_i and c_j can move before `basis` and `at_upper` stop being
        feasible / optimal for the LP of bounded().  The dict of basis_ranging plus b_side (m, 2): the bound the
        leaving variable leaves at (0 lower, 1 upper, -1 for an infinite end); NaN and -1 unless status is OPTIMAL."""
        return self._bounded_ranging(self.lib.lp_basis_bounded_ranging, A, b, c, lo, hi, basis, at_upper, maximize, eps)

    def bounded_ranging_large(self, A, b, c, lo, hi, basis, at_upper, maximize=False, eps=EPS):
        """lp_basis_bounded_ranging_large: bounded_ranging() on the tableau in HBM, at any shape bounded_large() runs
        (no basis_bounded_fits limit).  Returns the dict of bounded_ranging(), equal to it where both run."""
        return self._bounded_ranging(self.lib.lp_basis_bounded_ranging_large, A, b, c, lo, hi, basis, at_upper,
                                     maximize, eps)

    def _bounded_ranging(self, entry, A, b, c, lo, hi, basis, at_upper, maximize, eps):
        p = pack_lp(A, b, c, basis, lo, hi, at_upper)
        m, n, Af, b, c, basis, lo, hi, at_upper = p.m, p.n, p.A, p.b, p.c, p.basis, p.lo, p.hi, p.at_upper
        rhs, cost = np.zeros(2 * m), np.zeros(2 * n)
        rv, rs, cv = np.zeros(2 * m, np.int32), np.zeros(2 * m, np.int32), np.zeros(2 * n, np.int32)
        rc = self.check(entry(self.h, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper),
                              int(maximize), float(eps), _d(rhs), _i(rv), _i(rs), _d(cost), _i(cv)))
        return dict(_ranging_dict(rc, rhs, rv, cost, cv), b_side=rs.reshape(-1, 2))

    def bounded_ranging_batched(self, A, b, c, lo, hi, basis, at_upper, maximize=False, eps=EPS):
        """lp_basis_bounded_ranging_batched: arrays as bounded_duals_batched.  The dict of bounded_ranging with a
        leading batch axis; status (batch)."""
        p = pack_lp(A, b, c, basis, lo, hi, at_upper, batched=True)
        batch, m, n, Af, b, c = p.batch, p.m, p.n, p.A, p.b, p.c
        basis, lo, hi, at_upper = p.basis, p.lo, p.hi, p.at_upper
        rhs, cost = np.zeros((batch, 2 * m)), np.zeros((batch, 2 * n))
        rv, rs = np.zeros((batch, 2 * m), np.int32), np.zeros((batch, 2 * m), np.int32)
        cv = np.zeros((batch, 2 * n), np.int32)
        st = np.zeros(batch, dtype=np.int32)
        self.check(self.lib.lp_basis_bounded_ranging_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi),
                                                             _i(basis), _i(at_upper), int(maximize), float(eps),
                                                             _d(rhs), _i(rv), _i(rs), _d(cost), _i(cv), _i(st)))
        return dict(_ranging_dict(st, rhs, rv, cost, cv), b_side=rs.reshape(batch, -1, 2))

    def basis_bounded_fits(self, m, n):
        """lp_basis_bounded_fits: True if an m x n bounded LP runs the analysis kernel."""
        return bool(self.lib.lp_basis_bounded_fits(m, n))

    # ---- Farkas and unbounded-ray certificates of a bounded-variable LP at a basis --------------
    def basis_bounded_certificate(self, A, b, c, lo, hi, basis, at_upper, maximize=False, eps=EPS):
        """lp_basis_bounded_certificate: evidence for an infeasible or unbounded verdict of the LP of bounded() at
        `basis` (m; index n+i: the artificial of row i) and `at_upper` (n, 0/1), normally a result's, in the original
        variables.  The dict of basis_certificate: FARKAS proves f.b < min over the box of f^T A x, RAY is a direction
        of the box along which the objective improves without limit.  status OPTIMAL means the certificate was
        computed; SINGULAR for a singular crash or a repeated index, INFEASIBLE for some hi < lo (then NONE).  A bad
        bound, index or flag, a negative eps or a shape beyond basis_bounded_certificate_fits raises LPError with code
        BAD_ARG."""
        return self._basis_bounded_certificate(self.lib.lp_basis_bounded_certificate, A, b, c, lo, hi, basis, at_upper,
                                               maximize, eps)

    def basis_bounded_certificate_large(self, A, b, c, lo, hi, basis, at_upper, maximize=False, eps=EPS):
        """lp_basis_bounded_certificate_large: basis_bounded_certificate() on the tableau in HBM, at any shape
        bounded_large() and bounded_resolve_large() run (no basis_bounded_certificate_fits limit).  Returns the dict of
        basis_bounded_certificate(), equal to it where both run; refusals as there."""
        return self._basis_bounded_certificate(self.lib.lp_basis_bounded_certificate_large, A, b, c, lo, hi, basis,
                                               at_upper, maximize, eps)

    def _basis_bounded_certificate(self, entry, A, b, c, lo, hi, basis, at_upper, maximize, eps):
        p = pack_lp(A, b, c, basis, lo, hi, at_upper)
        m, n, Af, b, c, basis, lo, hi, at_upper = p.m, p.n, p.A, p.b, p.c, p.basis, p.lo, p.hi, p.at_upper
        kind, index = np.zeros(1, np.int32), np.zeros(1, np.int32)
        farkas, ray, value = np.zeros(m), np.zeros(n), np.zeros(1)
        rc = self.check(entry(self.h, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper),
                              int(maximize), float(eps), _i(kind), _d(farkas), _d(ray), _d(value), _i(index)))
        return dict(status=rc, kind=int(kind[0]), farkas=farkas, ray=ray, value=float(value[0]), index=int(index[0]))

    def basis_bounded_certificate_batched(self, A, b, c, lo, hi, basis, at_upper, maximize=False, eps=EPS,
                                          run_status=None):
        """lp_basis_bounded_certificate_batched: arrays as bounded_duals_batched; run_status (batch) or None, normally
        the statuses of the bounded_batched(), bounded_resolve_batched() or mip_bounded_solve_batched() call the bases
        come from: only LPs whose entry is INFEASIBLE or UNBOUNDED get a certificate (and keep the entry as their
        status when it was computed), the others keep their entry and get NONE.  The dict of
        basis_bounded_certificate with a leading batch axis; status, kind, value and index (batch)."""
        p = pack_lp(A, b, c, basis, lo, hi, at_upper, batched=True)
        batch, m, n, Af, b, c = p.batch, p.m, p.n, p.A, p.b, p.c
        basis, lo, hi, at_upper = p.basis, p.lo, p.hi, p.at_upper
        if run_status is not None:
            run_status = np.ascontiguousarray(run_status, dtype=np.int32).reshape(-1)
            if run_status.size != batch:
                raise ValueError("run_status must have batch entries")
        kind, index, st = np.zeros(batch, np.int32), np.zeros(batch, np.int32), np.zeros(batch, np.int32)
        farkas, ray, value = np.zeros((batch, m)), np.zeros((batch, n)), np.zeros(batch)
        self.check(self.lib.lp_basis_bounded_certificate_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _d(lo),
                                                                 _d(hi), _i(basis), _i(at_upper), _i(run_status),
                                                                 int(maximize), float(eps), _i(kind), _d(farkas),
                                                                 _d(ray), _d(value), _i(index), _i(st)))
        return dict(status=st, kind=kind, farkas=farkas, ray=ray, value=value, index=index)

    def basis_bounded_certificate_fits(self, m, n):
        """lp_basis_bounded_certificate_fits: True if an m x n bounded LP runs the certificate kernel."""
        return bool(self.lib.lp_basis_bounded_certificate_fits(m, n))

    # ---- parametric right-hand side and cost of a bounded-variable LP from an optimal basis -------
    def _bounded_parametric(self, fn, width, A, b, c, lo, hi, basis, at_upper, direction, t_max, maximize, eps,
                            max_breaks):
        p = pack_lp(A, b, c, basis, lo, hi, at_upper)
        m, n, Af, b, c, basis, lo, hi, at_upper = p.m, p.n, p.A, p.b, p.c, p.basis, p.lo, p.hi, p.at_upper
        direction = _direction(direction, n if width == "n" else m, "the direction must have %s entries" % width)
        mb = max(int(max_breaks), 0)
        nseg, t, obj, slope, enter, leave, bo, _ = _parametric_out(1, m, mb)
        side, up = np.zeros((1, mb + 1), np.int32), np.zeros(n, np.int32)
        rc = self.check(fn(self.h, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize),
                           _d(direction), float(t_max), float(eps), int(max_breaks), _i(nseg), _d(t), _d(obj),
                           _d(slope), _i(enter), _i(leave), _i(side), _i(bo), _i(up)))
        ns = int(nseg[0])
        return dict(status=rc, t=t[0, :ns + 1] if ns else t[0, :0], obj=obj[0, :ns + 1] if ns else obj[0, :0],
                    slope=slope[0, :ns], enter=enter[0, :ns], leave=leave[0, :ns], side=side[0, :ns], basis=bo[0],
                    at_upper=up)

    def _bounded_parametric_batched(self, fn, width, A, b, c, lo, hi, basis, at_upper, direction, t_max, maximize, eps,
                                    max_breaks, run_status):
        p = pack_lp(A, b, c, basis, lo, hi, at_upper, batched=True)
        batch, m, n, Af, b, c = p.batch, p.m, p.n, p.A, p.b, p.c
        basis, lo, hi, at_upper = p.basis, p.lo, p.hi, p.at_upper
        direction = _direction(direction, batch * (n if width == "n" else m),
                               "the direction must have %s entries per LP" % width)
        if run_status is not None:
            run_status = np.ascontiguousarray(run_status, dtype=np.int32).reshape(-1)
            if run_status.size != batch:
                raise ValueError("run_status must have batch entries")
        mb = max(int(max_breaks), 0)
        out = _parametric_out(batch, m, mb)
        nseg, t, obj, slope, enter, leave, bo, st = out
        side, up = np.zeros((batch, mb + 1), np.int32), np.zeros((batch, n), np.int32)
        self.check(fn(self.h, batch, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper),
                      _i(run_status), int(maximize), _d(direction), float(t_max), float(eps), int(max_breaks), _i(nseg),
                      _d(t), _d(obj), _d(slope), _i(enter), _i(leave), _i(side), _i(bo), _i(up), _i(st)))
        return dict(_parametric_dict(out), side=side, at_upper=up)

    def bounded_parametric(self, A, b, c, lo, hi, basis, at_upper, d, t_max=np.inf, maximize=True, eps=EPS,
                           max_breaks=MAX_BREAKS):
        """lp_basis_bounded_parametric: the optimal value of the LP of bounded() along b + t d for t in [0, t_max] from
        the optimal `basis` (m) and `at_upper` (n, 0/1), normally a result's.  The dict of basis_parametric plus side
        (nseg): the bound at which leave[k] stops (0 lower, 1 upper, -1 on a last segment that reached t_max) and
        at_upper (n): the flags that go with the final basis.  status OPTIMAL (reached t_max), INFEASIBLE (infeasible
        past t[-1], or some hi < lo: empty arrays), ITER_LIMIT (max_breaks pivots done) or SINGULAR (empty arrays).  A
        basis that is not optimal at t = 0, a bad bound, index or flag, t_max < 0, eps < 0, max_breaks < 0 or a shape
        beyond bounded_parametric_fits raises LPError with code BAD_ARG."""
        return self._bounded_parametric(self.lib.lp_basis_bounded_parametric, "m", A, b, c, lo, hi, basis, at_upper, d,
                                        t_max, maximize, eps, max_breaks)

    def bounded_parametric_batched(self, A, b, c, lo, hi, basis, at_upper, d, t_max=np.inf, maximize=True, eps=EPS,
                                   max_breaks=MAX_BREAKS, run_status=None):
        """lp_basis_bounded_parametric_batched: arrays as bounded_duals_batched, d (batch, m); run_status (batch) or
        None, normally the statuses of the bounded_batched() or bounded_resolve_batched() call the bases come from: an
        LP whose entry is not OPTIMAL keeps it and gets nseg 0.  The dict of basis_parametric_batched plus side
        (batch, max_breaks+1) and at_upper (batch, n), padded with NaN / -1 past each path."""
        return self._bounded_parametric_batched(self.lib.lp_basis_bounded_parametric_batched, "m", A, b, c, lo, hi,
                                                basis, at_upper, d, t_max, maximize, eps, max_breaks, run_status)

    def bounded_parametric_cost(self, A, b, c, lo, hi, basis, at_upper, g, t_max=np.inf, maximize=True, eps=EPS,
                                max_breaks=MAX_BREAKS):
        """lp_basis_bounded_parametric_cost: the optimal value of the LP of bounded() along c + t g for t in
        [0, t_max].  The dict of bounded_parametric; a bound flip is a breakpoint with enter[k] == leave[k] and side[k]
        the bound flipped to.  status OPTIMAL (reached t_max), UNBOUNDED (unbounded past t[-1]), ITER_LIMIT
        (max_breaks pivots and flips done), INFEASIBLE (some hi < lo: empty arrays) or SINGULAR (empty arrays)."""
        return self._bounded_parametric(self.lib.lp_basis_bounded_parametric_cost, "n", A, b, c, lo, hi, basis,
                                        at_upper, g, t_max, maximize, eps, max_breaks)

    def bounded_parametric_cost_batched(self, A, b, c, lo, hi, basis, at_upper, g, t_max=np.inf, maximize=True,
                                        eps=EPS, max_breaks=MAX_BREAKS, run_status=None):
        """lp_basis_bounded_parametric_cost_batched: as bounded_parametric_batched with g (batch, n)."""
        return self._bounded_parametric_batched(self.lib.lp_basis_bounded_parametric_cost_batched, "n", A, b, c, lo,
                                                hi, basis, at_upper, g, t_max, maximize, eps, max_breaks, run_status)

    def bounded_parametric_large(self, A, b, c, lo, hi, basis, at_upper, d, t_max=np.inf, maximize=True, eps=EPS,
                                 max_breaks=MAX_BREAKS):
        """lp_basis_bounded_parametric_large: bounded_parametric() on the tableau in HBM, at any shape bounded_large()
        and bounded_resolve_large() run (one selector + one update launch per breakpoint).  Same arguments, dict and
        statuses; no bounded_parametric_fits limit (m <= 6638 for the selector's LDS)."""
        return self._bounded_parametric(self.lib.lp_basis_bounded_parametric_large, "m", A, b, c, lo, hi, basis,
                                        at_upper, d, t_max, maximize, eps, max_breaks)

    def bounded_parametric_cost_large(self, A, b, c, lo, hi, basis, at_upper, g, t_max=np.inf, maximize=True, eps=EPS,
                                      max_breaks=MAX_BREAKS):
        """lp_basis_bounded_parametric_cost_large: bounded_parametric_cost() on the tableau in HBM, at any shape
        bounded_large() and bounded_resolve_large() run.  Same arguments, dict and statuses; no
        bounded_parametric_cost_fits limit (m <= 3982 for the selector's LDS)."""
        return self._bounded_parametric(self.lib.lp_basis_bounded_parametric_cost_large, "n", A, b, c, lo, hi, basis,
                                        at_upper, g, t_max, maximize, eps, max_breaks)

    def bounded_parametric_fits(self, m, n):
        """lp_basis_bounded_parametric_fits: True if an m x n bounded LP runs the RHS path's kernel."""
        return bool(self.lib.lp_basis_bounded_parametric_fits(m, n))

    def bounded_parametric_cost_fits(self, m, n):
        """lp_basis_bounded_parametric_cost_fits: True if an m x n bounded LP runs the cost path's kernel."""
        return bool(self.lib.lp_basis_bounded_parametric_cost_fits(m, n))

    # ---- branch-and-bound over the bounds of a bounded-variable LP -----------------------------
    def mip_bounded_solve(self, A, b, c, lo, hi, basis, at_upper, integer, maximize=True, n_orig=None, eps=EPS,
                          int_tol=INT_TOL, gap=GAP, max_depth=MAX_DEPTH_BOUNDED, max_nodes=MAX_NODES,
                          max_iter=MAX_ITER, dual_ratio=None):
        """lp_mip_bounded_solve: opt c.x, A x = b, lo <= x <= hi, x_j integral where integer[j] (n entries, 0/1,
        j < n_orig), searched by changing bounds from `basis` (m) and `at_upper` (n), normally bounded()'s result.
        dict(status, found, x (n_orig), obj, bound, stats (nodes, dual pivots, primal pivots, bound flips, deepest
        level)); x and obj NaN without an incumbent.  A start that is no valid one, a fractional bound on a marked
        column, a bad argument or a shape beyond mip_bounded_fits raises LPError with code BAD_ARG.
        dual_ratio ("textbook", "long_step" or a DUAL_RATIO_* value; None: the call made without it) goes through
        lp_mip_bounded_solve_ratio_ex and picks the ratio test of every dual loop of the search; under "long_step"
        stats[3] counts the dual loops' flips too."""
        p = pack_lp(A, b, c, basis, lo, hi, at_upper)
        m, n, Af, b, c, basis, lo, hi, at_upper = p.m, p.n, p.A, p.b, p.c, p.basis, p.lo, p.hi, p.at_upper
        n_orig = n if n_orig is None else int(n_orig)
        integer = _mask(integer, n)
        x, obj, bound, found, stats, _ = _mip_out(1, n_orig, 5)
        args = (self.h, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize), n_orig,
                _i(integer), float(eps), float(int_tol), float(gap), int(max_depth), int(max_nodes), int(max_iter),
                _d(x), _d(obj), _d(bound), _i(found), _i(stats))
        if dual_ratio is None:
            rc = self.check(self.lib.lp_mip_bounded_solve(*args))
        else:
            rc = self.check(self.lib.lp_mip_bounded_solve_ratio_ex(*args, dual_ratio_id(dual_ratio)))
        return dict(status=rc, found=int(found[0]), x=x[0], obj=float(obj[0]), bound=float(bound[0]),
                    stats=tuple(int(v) for v in stats[0]))

    def mip_bounded_solve_batched(self, A, b, c, lo, hi, integer, basis=None, at_upper=None, root_status=None,
                                  maximize=True, n_orig=None, eps=EPS, int_tol=INT_TOL, gap=GAP,
                                  max_depth=MAX_DEPTH_BOUNDED, max_nodes=MAX_NODES, max_iter=MAX_ITER,
                                  dual_ratio=None):
        """lp_mip_bounded_solve_batched: arrays as bounded_resolve_batched(), one mask (n); root_status (batch) or
        None.  basis=None runs bounded_batched() first and searches from its bases and flags, its statuses passed as
        root_status: an LP whose cold solve is not OPTIMAL keeps that status.  dict(status, found, obj, bound (batch),
        x (batch, n_orig), stats (batch, 5)).  dual_ratio as mip_bounded_solve() (lp_mip_bounded_solve_batched_ratio_ex);
        the cold solve of the basis=None chain has no dual loop and is the same under every value."""
        n_orig = np.shape(A)[2] if n_orig is None else int(n_orig)
        if basis is None:
            if at_upper is not None or root_status is not None:
                raise ValueError("at_upper and root_status go with basis")
            cold = self.bounded_batched(A, b, c, lo, hi, maximize, n_orig, eps, max_iter)
            root_status = cold["status"]
            ok = root_status == OPTIMAL   # (an unfinished LP's basis may hold artificials: not read, but checked)
            basis = np.where(ok[:, None], cold["basis"], 0)
            at_upper = np.where(ok[:, None], cold["at_upper"], 0)
        p = pack_lp(A, b, c, basis, lo, hi, at_upper, batched=True)
        batch, m, n, Af, b, c = p.batch, p.m, p.n, p.A, p.b, p.c
        basis, lo, hi, at_upper = p.basis, p.lo, p.hi, p.at_upper
        if root_status is not None:
            root_status = np.ascontiguousarray(root_status, dtype=np.int32).reshape(-1)
            if root_status.size != batch:
                raise ValueError("root_status must have batch entries")
        integer = _mask(integer, n)
        out = _mip_out(batch, n_orig, 5)
        x, obj, bound, found, stats, st = out
        args = (self.h, batch, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper),
                _i(root_status), int(maximize), n_orig, _i(integer), float(eps),
                float(int_tol), float(gap), int(max_depth), int(max_nodes), int(max_iter), _d(x), _d(obj), _d(bound),
                _i(found), _i(stats), _i(st))
        if dual_ratio is None:
            self.check(self.lib.lp_mip_bounded_solve_batched(*args))
        else:
            self.check(self.lib.lp_mip_bounded_solve_batched_ratio_ex(*args, dual_ratio_id(dual_ratio)))
        return _mip_dict(out)

    def mip_bounded_solve_large(self, A, b, c, lo, hi, basis, at_upper, integer, maximize=True, n_orig=None, eps=EPS,
                                int_tol=INT_TOL, gap=GAP, max_depth=MAX_DEPTH_BOUNDED, max_nodes=MAX_NODES,
                                max_iter=MAX_ITER, snapshots=None, dual_ratio=None):
        """lp_mip_bounded_solve_large: mip_bounded_solve() on the tableau in HBM, at any shape
        bounded_resolve_large() runs (no mip_bounded_fits limit; m <= 9960).  Arguments, the dict returned and the
        refusals are mip_bounded_solve()'s, and at a shape that also fits LDS so is every value.
        snapshots = K (an int in [0, 1024]): lp_mip_bounded_solve_large_ex, which keeps up to min(K, max_depth)
        tableau snapshots on the device (mip_bounded_snapshot_bytes says how large) and starts a second child from its
        parent's final tableau where its level's snapshot is still there; stats then has seven entries, the last two
        the second children restored and rebuilt.  K = 0 equals the call without the argument.
        dual_ratio as mip_bounded_solve(): lp_mip_bounded_solve_large_ratio_ex (with snapshots=None: no snapshots, and
        the five counters are returned)."""
        p = pack_lp(A, b, c, basis, lo, hi, at_upper)
        m, n, Af, b, c, basis, lo, hi, at_upper = p.m, p.n, p.A, p.b, p.c, p.basis, p.lo, p.hi, p.at_upper
        n_orig = n if n_orig is None else int(n_orig)
        integer = _mask(integer, n)
        nstats = 5 if snapshots is None else 7
        x, obj, bound, found, stats, _ = _mip_out(1, n_orig, nstats if dual_ratio is None else 7)
        args = (self.h, _d(Af), m, n, _d(b), _d(c), _d(lo), _d(hi), _i(basis), _i(at_upper), int(maximize), n_orig,
                _i(integer), float(eps), float(int_tol), float(gap), int(max_depth), int(max_nodes), int(max_iter),
                _d(x), _d(obj), _d(bound), _i(found), _i(stats))
        if dual_ratio is not None:
            rc = self.check(self.lib.lp_mip_bounded_solve_large_ratio_ex(*args, int(snapshots or 0),
                                                                         dual_ratio_id(dual_ratio)))
        elif snapshots is None:
            rc = self.check(self.lib.lp_mip_bounded_solve_large(*args))
        else:
            rc = self.check(self.lib.lp_mip_bounded_solve_large_ex(*args, int(snapshots)))
        return dict(status=rc, found=int(found[0]), x=x[0], obj=float(obj[0]), bound=float(bound[0]),
                    stats=tuple(int(v) for v in stats[0][:nstats]))

    def mip_bounded_snapshot_bytes(self, m, n, snapshots):
        """lp_mip_bounded_snapshot_bytes: the device bytes `snapshots` tableau snapshots of an m x n problem take."""
        out = C.c_uint64(0)
        rc = self.lib.lp_mip_bounded_snapshot_bytes(int(m), int(n), int(snapshots), C.byref(out))
        if rc != OPTIMAL:   # (a host call: the context holds no message for it)
            raise LPError(rc, "lp_mip_bounded_snapshot_bytes: bad dimensions or snapshots outside [0, 1024]")
        return int(out.value)

    def mip_bounded_fits(self, m, n, max_depth=MAX_DEPTH_BOUNDED):
        """lp_mip_bounded_fits: True if an m x n bounded problem searched to max_depth fits one CU's LDS."""
        return bool(self.lib.lp_mip_bounded_fits(m, n, max_depth))

    # ---- Farkas and unbounded-ray certificates at a basis -------------------------------------
    def basis_certificate(self, A, b, c, basis, maximize=True, eps=EPS):
        """lp_basis_certificate: evidence for an infeasible or unbounded verdict at `basis` (index n+i: the
        artificial of row i).  dict(status, kind (CERT_NONE / CERT_FARKAS / CERT_RAY), farkas (m), ray (n), value,
        index): farkas NaN unless the kind is FARKAS, ray NaN unless it is RAY.  status OPTIMAL means the
        certificate was computed; SINGULAR for a singular crash or a repeated index.  An index out of range or a
        negative eps raises LPError with code BAD_ARG."""
        p = pack_lp(A, b, c, basis)
        m, n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        kind, index = np.zeros(1, np.int32), np.zeros(1, np.int32)
        farkas, ray, value = np.zeros(m), np.zeros(n), np.zeros(1)
        rc = self.check(self.lib.lp_basis_certificate(self.h, _d(Af), m, n, _d(b), _d(c), _i(basis), int(maximize),
                                                      float(eps), _i(kind), _d(farkas), _d(ray), _d(value),
                                                      _i(index)))
        return dict(status=rc, kind=int(kind[0]), farkas=farkas, ray=ray, value=float(value[0]),
                    index=int(index[0]))

    def basis_certificate_batched(self, A, b, c, basis, maximize=True, eps=EPS):
        """lp_basis_certificate_batched: A (batch, m, n), b (batch, m), c (batch, n), basis (batch, m).  The dict
        of basis_certificate with a leading batch axis; status, kind, value and index (batch)."""
        p = pack_lp(A, b, c, basis, batched=True)
        batch, m, n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        kind, index, st = np.zeros(batch, np.int32), np.zeros(batch, np.int32), np.zeros(batch, np.int32)
        farkas, ray, value = np.zeros((batch, m)), np.zeros((batch, n)), np.zeros(batch)
        self.check(self.lib.lp_basis_certificate_batched(self.h, batch, _d(Af), m, n, _d(b), _d(c), _i(basis),
                                                         int(maximize), float(eps), _i(kind), _d(farkas), _d(ray),
                                                         _d(value), _i(index), _i(st)))
        return dict(status=st, kind=kind, farkas=farkas, ray=ray, value=value, index=index)

    def basis_certificate_fits(self, m, n):
        """lp_basis_certificate_fits: True if an m x n LP runs the one-LP-per-workgroup kernel."""
        return bool(self.lib.lp_basis_certificate_fits(m, n))

    def simplex_solve_batched(self, A, b, c, basis, maximize=True, n_orig=None, eps=EPS,
                              max_iter=MAX_ITER, pivot_rule="dantzig"):
        """A: (batch, m, n); b: (batch, m); c: (batch, n); basis: (batch, m)."""
        p = pack_lp(A, b, c, basis, batched=True)
        batch, m, n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        n_orig = n if n_orig is None else n_orig
        x = np.zeros((batch, n_orig))
        bo = np.zeros((batch, m), dtype=np.int32)
        obj = np.full(batch, np.nan)
        it = np.zeros(batch, dtype=np.int32)
        st = np.zeros(batch, dtype=np.int32)
        self.check(self.lib.lp_simplex_solve_batched_ex(self.h, batch, _d(Af), m, n, _d(b), _d(c),
                                                        _i(basis), int(maximize), n_orig, eps,
                                                        max_iter, _d(x), _i(bo), _d(obj), _i(it),
                                                        _i(st), pivot_rule_id(pivot_rule)))
        return dict(status=st, x=x, basis=bo, obj=obj, iters=it)

    def batched_problem(self, A, b, c, basis, maximize=True, n_orig=None):
        return BatchedProblem(self, A, b, c, basis, maximize, n_orig)

    def two_phase_batched(self, A, b, c, maximize=False, n_orig=None, eps=EPS, max_iter=MAX_ITER,
                          pivot_rule="dantzig"):
        """lp_simplex_two_phase_batched: A (batch, m, n), b (batch, m), c (batch, n), no basis;
        per LP exactly two_phase().  iters: (batch, 3) = phase I, drive-out, phase II."""
        p = pack_lp(A, b, c, batched=True)
        batch, m, n, Af, b, c = p.batch, p.m, p.n, p.A, p.b, p.c
        n_orig = n if n_orig is None else n_orig
        x = np.zeros((batch, n_orig))
        bo = np.full((batch, m), -1, dtype=np.int32)
        obj = np.full(batch, np.nan)
        it = np.zeros((batch, 3), dtype=np.int32)
        st = np.zeros(batch, dtype=np.int32)
        self.check(self.lib.lp_simplex_two_phase_batched_ex(self.h, batch, _d(Af), m, n, _d(b), _d(c),
                                                            int(maximize), n_orig, eps, max_iter, _d(x),
                                                            _i(bo), _d(obj), _i(it), _i(st),
                                                            pivot_rule_id(pivot_rule)))
        return dict(status=st, x=x, basis=bo, obj=obj, iters=it)

    def batched_two_phase_problem(self, A, b, c, maximize=False, n_orig=None):
        """Device-resident two-phase batch (lp_batched_two_phase_upload)."""
        return BatchedProblem(self, A, b, c, None, maximize, n_orig)

    # ---- enumeration ---------------------------------------------------------------------
    def enum_solve(self, A, b, c, maximize=True, n_orig=None):
        p = pack_lp(A, b, c)
        m, n, Af, b, c = p.m, p.n, p.A, p.b, p.c
        n_orig = n if n_orig is None else n_orig
        x = np.zeros(n_orig)
        bo = np.zeros(m, dtype=np.int32)
        rank = C.c_uint64(0)
        obj = C.c_double(float("nan"))
        counts = (C.c_uint64 * 3)()
        rc = self.check(self.lib.lp_enum_solve(self.h, _d(Af), m, n, _d(b), _d(c), int(maximize),
                                               n_orig, _d(x), _i(bo), C.byref(rank), C.byref(obj),
                                               counts))
        return dict(status=rc, x=x, basis=bo, rank=int(rank.value), obj=obj.value,
                    counts=[int(v) for v in counts])

    def enum_problem(self, A, b, c, maximize=True):
        return EnumProblem(self, A, b, c, maximize)


class SimplexProblem:
    """Device-resident tableau (lp_simplex_problem)."""

    def __init__(self, ctx, A, b, c, basis, maximize=True, n_orig=None):
        p = pack_lp(A, b, c, basis)
        self.m, self.n, Af, b, c, basis = p.m, p.n, p.A, p.b, p.c, p.basis
        self.ctx, self.n_orig = ctx, self.n if n_orig is None else n_orig
        h = _vp()
        ctx.check(ctx.lib.lp_simplex_upload(ctx.h, _d(Af), self.m, self.n, _d(b), _d(c), _i(basis),
                                            int(maximize), self.n_orig, C.byref(h)))
        self.h = h

    def reset(self):
        self.ctx.check(self.ctx.lib.lp_simplex_reset(self.h))

    def set_pivot_rule(self, rule):
        """"dantzig" (the default after upload), "bland" or "devex", for the following runs."""
        self.ctx.check(self.ctx.lib.lp_simplex_set_pivot_rule(self.h, pivot_rule_id(rule)))

    def profile(self, on=True):
        self.ctx.check(self.ctx.lib.lp_simplex_profile(self.h, int(on)))

    def run(self, eps=EPS, max_iter=MAX_ITER, algo=SIMPLEX_AUTO):
        st = SimplexStats()
        rc = self.ctx.check(self.ctx.lib.lp_simplex_run(self.h, eps, max_iter, algo, C.byref(st)))
        return rc, st

    def resolve(self, eps=EPS, max_iter=MAX_ITER):
        """lp_simplex_resolve_run on the current tableau: (status, stats, (dual pivots, primal pivots))."""
        st = SimplexStats()
        it = np.zeros(2, dtype=np.int32)
        rc = self.ctx.check(self.ctx.lib.lp_simplex_resolve_run(self.h, eps, max_iter, _i(it), C.byref(st)))
        return rc, st, (int(it[0]), int(it[1]))

    def download(self, trace_cap=0, want_tableau=False):
        x = np.zeros(self.n_orig)
        bo = np.zeros(self.m, dtype=np.int32)
        obj = C.c_double(float("nan"))
        te = np.full(max(trace_cap, 1), -1, dtype=np.int32)
        tl = np.full(max(trace_cap, 1), -1, dtype=np.int32)
        tab = np.zeros((self.m + 1, self.n + 1)) if want_tableau else None
        self.ctx.check(self.ctx.lib.lp_simplex_download(self.h, _d(x), _i(bo), C.byref(obj), _i(te),
                                                        _i(tl), trace_cap, _d(tab)))
        return dict(x=x, basis=bo, obj=obj.value, trace_enter=te[:trace_cap],
                    trace_leave=tl[:trace_cap], tableau=tab)

    def row(self, row):
        """Row `row` of the current tableau (m = reduced costs): n + 1 doubles."""
        out = np.zeros(self.n + 1)
        self.ctx.check(self.ctx.lib.lp_simplex_row(self.h, int(row), _d(out)))
        return out

    def force_pivot(self, row, col):
        return self.ctx.check(self.ctx.lib.lp_simplex_force_pivot(self.h, int(row), int(col)))

    def bench_update(self, row, col, iters):
        ms = C.c_float(0.0)
        self.ctx.check(self.ctx.lib.lp_bench_rank1_update(self.h, row, col, iters, C.byref(ms)))
        return ms.value

    def bench_update_rankj(self, iters):
        ms = C.c_float(0.0)
        piv = C.c_int(0)
        self.ctx.check(self.ctx.lib.lp_bench_rankj_update(self.h, iters, C.byref(ms), C.byref(piv)))
        return ms.value, piv.value

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.lp_simplex_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BatchedProblem:
    def __init__(self, ctx, A, b, c, basis, maximize=True, n_orig=None, resolve=False):
        self.two_phase = basis is None   # no starting basis: the two-phase flow
        p = pack_lp(A, b, c, basis, batched=True)
        self.batch, self.m, self.n, Af, b, c, basis = p.batch, p.m, p.n, p.A, p.b, p.c, p.basis
        self.ctx, self.n_orig = ctx, self.n if n_orig is None else n_orig
        h = _vp()
        if resolve:
            ctx.check(ctx.lib.lp_batched_resolve_upload(ctx.h, self.batch, _d(Af), self.m, self.n, _d(b), _d(c),
                                                        _i(basis), int(maximize), self.n_orig, C.byref(h)))
        elif self.two_phase:
            ctx.check(ctx.lib.lp_batched_two_phase_upload(ctx.h, self.batch, _d(Af), self.m, self.n, _d(b),
                                                          _d(c), int(maximize), self.n_orig, C.byref(h)))
        else:
            ctx.check(ctx.lib.lp_batched_upload(ctx.h, self.batch, _d(Af), self.m, self.n, _d(b), _d(c),
                                                _i(basis), int(maximize), self.n_orig, C.byref(h)))
        self.h = h

    def set_pivot_rule(self, rule):
        """"dantzig" (the default after upload), "bland" or "devex", for the following runs."""
        self.ctx.check(self.ctx.lib.lp_batched_set_pivot_rule(self.h, pivot_rule_id(rule)))

    def run(self, eps=EPS, max_iter=MAX_ITER):
        ms = C.c_float(0.0)
        self.ctx.check(self.ctx.lib.lp_batched_run(self.h, eps, max_iter, C.byref(ms)))
        return ms.value

    def download(self):
        x = np.zeros((self.batch, self.n_orig))
        bo = np.zeros((self.batch, self.m), dtype=np.int32)
        obj = np.full(self.batch, np.nan)
        it = np.zeros(self.batch, dtype=np.int32)
        st = np.zeros(self.batch, dtype=np.int32)
        self.ctx.check(self.ctx.lib.lp_batched_download(self.h, _d(x), _i(bo), _d(obj), _i(it),
                                                        _i(st)))
        return dict(status=st, x=x, basis=bo, obj=obj, iters=it)

    def phase_iters(self):
        """(batch, 3) pivot counts of the last run: phase I, drive-out, phase II (two-phase batches)."""
        it = np.zeros((self.batch, 3), dtype=np.int32)
        self.ctx.check(self.ctx.lib.lp_batched_phase_iters(self.h, _i(it)))
        return it

    def set_start(self, b=None, basis=None):
        """Re-solve batches: new right-hand sides (batch, m) and/or starting bases (batch, m); A and c stay."""
        b = None if b is None else _f64(b).reshape(-1)
        basis = None if basis is None else np.ascontiguousarray(basis, dtype=np.int32).reshape(-1)
        for a in (b, basis):
            if a is not None and a.size != self.batch * self.m:
                raise ValueError(f"set_start: expected {self.batch * self.m} entries, got {a.size}")
        self.ctx.check(self.ctx.lib.lp_batched_set_start(self.h, _d(b), _i(basis)))

    def resolve_iters(self):
        """(batch, 2) pivot counts of the last run: dual, primal (re-solve batches)."""
        it = np.zeros((self.batch, 2), dtype=np.int32)
        self.ctx.check(self.ctx.lib.lp_batched_resolve_iters(self.h, _i(it)))
        return it

    def duals(self):
        """lp_batched_duals after run(): dict(status (batch), y (batch, m), d (batch, n), w (batch)) at each LP's
        final basis; LPs whose run status is not OPTIMAL keep it and get NaN."""
        y, d, w = np.zeros((self.batch, self.m)), np.zeros((self.batch, self.n)), np.zeros(self.batch)
        st = np.zeros(self.batch, dtype=np.int32)
        self.ctx.check(self.ctx.lib.lp_batched_duals(self.h, _d(y), _d(d), _d(w), _i(st)))
        return dict(status=st, y=y, d=d, w=w)

    def ranging(self, eps=EPS):
        """lp_batched_ranging after run(): the dict of Context.basis_ranging_batched at each LP's final basis and the
        handle's sense; LPs whose run status is not OPTIMAL keep it and get NaN."""
        B, m, n = self.batch, self.m, self.n
        rhs, cost = np.zeros((B, 2 * m)), np.zeros((B, 2 * n))
        rv, cv = np.zeros((B, 2 * m), np.int32), np.zeros((B, 2 * n), np.int32)
        st = np.zeros(B, dtype=np.int32)
        self.ctx.check(self.ctx.lib.lp_batched_ranging(self.h, float(eps), _d(rhs), _i(rv), _d(cost), _i(cv), _i(st)))
        return _ranging_dict(st, rhs, rv, cost, cv)

    def certificates(self, eps=EPS):
        """lp_batched_certificates after run(): the dict of Context.basis_certificate_batched at each LP's final
        basis and the handle's sense.  Only LPs whose run ended INFEASIBLE or UNBOUNDED get a certificate; status
        holds the run status (SINGULAR if the certificate's crash fails)."""
        B, m, n = self.batch, self.m, self.n
        kind, index, st = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        farkas, ray, value = np.zeros((B, m)), np.zeros((B, n)), np.zeros(B)
        self.ctx.check(self.ctx.lib.lp_batched_certificates(self.h, float(eps), _i(kind), _d(farkas), _d(ray),
                                                            _d(value), _i(index), _i(st)))
        return dict(status=st, kind=kind, farkas=farkas, ray=ray, value=value, index=index)

    def parametric(self, d, t_max=np.inf, eps=EPS, max_breaks=MAX_BREAKS):
        """lp_batched_parametric after run(): the dict of Context.basis_parametric_batched from each LP's final basis,
        d (batch, m), with the handle's sense; LPs whose run status is not OPTIMAL keep it and get nseg 0."""
        d = _direction(d, self.batch * self.m, "parametric: expected {size} direction entries, got {got}")
        out = _parametric_out(self.batch, self.m, max(int(max_breaks), 0))
        nseg, t, obj, slope, enter, leave, bo, st = out
        self.ctx.check(self.ctx.lib.lp_batched_parametric(self.h, _d(d), float(t_max), float(eps), int(max_breaks),
                                                          _i(nseg), _d(t), _d(obj), _d(slope), _i(enter), _i(leave),
                                                          _i(bo), _i(st)))
        return _parametric_dict(out)

    def parametric_cost(self, g, t_max=np.inf, eps=EPS, max_breaks=MAX_BREAKS):
        """lp_batched_parametric_cost after run(): the dict of Context.basis_parametric_cost_batched from each LP's
        final basis, g (batch, n), with the handle's sense; LPs whose run status is not OPTIMAL keep it and get
        nseg 0."""
        g = _direction(g, self.batch * self.n,
                       "parametric_cost: expected {size} cost direction entries, got {got}")
        out = _parametric_out(self.batch, self.m, max(int(max_breaks), 0))
        nseg, t, obj, slope, enter, leave, bo, st = out
        self.ctx.check(self.ctx.lib.lp_batched_parametric_cost(self.h, _d(g), float(t_max), float(eps),
                                                               int(max_breaks), _i(nseg), _d(t), _d(obj), _d(slope),
                                                               _i(enter), _i(leave), _i(bo), _i(st)))
        return _parametric_dict(out)

    def mip(self, integer, eps=EPS, int_tol=INT_TOL, gap=GAP, max_depth=MAX_DEPTH, max_nodes=MAX_NODES,
            max_iter=MAX_ITER):
        """lp_batched_mip after run(): the dict of Context.mip_batched from each LP's final basis with the handle's
        sense; LPs whose run status is not OPTIMAL keep it (found 0, NaN)."""
        integer = _mask(integer, self.n)
        out = _mip_out(self.batch, self.n_orig)
        x, obj, bound, found, stats, st = out
        self.ctx.check(self.ctx.lib.lp_batched_mip(self.h, _i(integer), float(eps), float(int_tol), float(gap),
                                                   int(max_depth), int(max_nodes), int(max_iter), _d(x), _d(obj),
                                                   _d(bound), _i(found), _i(stats), _i(st)))
        return _mip_dict(out)

    def path(self):
        """1: one LP per workgroup on the GPU; 0: the per-LP fallback."""
        return self.ctx.check(self.ctx.lib.lp_batched_path(self.h))

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.lp_batched_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class EnumProblem:
    """Device-resident enumeration problem (lp_enum_problem)."""

    def __init__(self, ctx, A, b, c, maximize=True):
        p = pack_lp(A, b, c)
        self.m, self.n, Af, b, c = p.m, p.n, p.A, p.b, p.c
        self.ctx, self.maximize = ctx, bool(maximize)
        h = _vp()
        ctx.check(ctx.lib.lp_enum_upload(ctx.h, _d(Af), self.m, self.n, _d(b), _d(c),
                                         int(maximize), C.byref(h)))
        self.h = h
        self.total = int(ctx.lib.lp_binom(self.n, self.m))

    def range(self, begin, end, algo=ENUM_AUTO):
        z = C.c_double(0.0)
        counts = (C.c_uint64 * 3)()
        st = EnumStats()
        rc = self.ctx.check(self.ctx.lib.lp_enum_range(self.h, begin, end, algo, C.byref(z), counts,
                                                       C.byref(st)))
        return rc, z.value, [int(v) for v in counts], st

    def first_within(self, begin, end, zstar, tol=1e-9):
        r = C.c_uint64(0)
        self.ctx.check(self.ctx.lib.lp_enum_first_within(self.h, begin, end, zstar, tol,
                                                         C.byref(r)))
        return int(r.value)

    def solve_sharded(self, comm=None, n_orig=None, want_vertex=True):
        """lp_enum_solve_sharded: this participant's shard of the rank space + the one exchange.
        comm: a Comm (or None = single participant).  Blocks until every participant has called.
        want_vertex=False: rank, objective and counts only (no vertex kernel)."""
        n_orig = self.n if n_orig is None else n_orig
        x = np.zeros(n_orig)
        bo = np.zeros(self.m, dtype=np.int32)
        rank = C.c_uint64(0)
        obj = C.c_double(float("nan"))
        counts = (C.c_uint64 * 3)()
        rc = self.ctx.check(self.ctx.lib.lp_enum_solve_sharded(
            comm.h if comm is not None else None, self.h, n_orig, _d(x) if want_vertex else None,
            _i(bo) if want_vertex else None, C.byref(rank), C.byref(obj), counts))
        return dict(status=rc, x=x, basis=bo, rank=int(rank.value), obj=obj.value,
                    counts=[int(v) for v in counts])

    @property
    def exact_division(self):
        """True once the leaf kernels divide plainly (include/simplexmethod_amd.h: lp_enum_exact_division)."""
        return bool(self.ctx.lib.lp_enum_exact_division(self.h))

    def vertex(self, rank, n_orig=None):
        n_orig = self.n if n_orig is None else n_orig
        x = np.zeros(n_orig)
        bo = np.zeros(self.m, dtype=np.int32)
        obj = C.c_double(float("nan"))
        verdict = C.c_int(-1)
        self.ctx.check(self.ctx.lib.lp_enum_vertex(self.h, rank, n_orig, _d(x), _i(bo),
                                                   C.byref(obj), C.byref(verdict)))
        return dict(x=x, basis=bo, obj=obj.value, verdict=verdict.value)

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.lp_enum_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm:
    """lp_comm: the exchange of the sharded enumeration (one per participant)."""

    def __init__(self, handle, lib):
        self.h, self.lib = handle, lib

    @staticmethod
    def unique_id():
        """128 bytes for Comm.rccl (rank 0 creates them and hands them to the other participants)."""
        buf = C.create_string_buffer(128)
        if load().lp_comm_unique_id(buf) != OPTIMAL:
            raise LPError(BAD_ARG, "RCCL is not available (lp_comm_unique_id)")
        return buf.raw

    @staticmethod
    def rccl(ctx, rank, world, unique_id):
        """Collective: every participant calls it with the same id (ncclCommInitRank)."""
        h = _vp()
        ctx.check(ctx.lib.lp_comm_create_rccl(ctx.h, rank, world, C.c_char_p(unique_id), C.byref(h)))
        return Comm(h, ctx.lib)

    @staticmethod
    def local(world):
        """`world` communicators for host threads of this process (exchange through host memory)."""
        lib = load()
        arr = (_vp * world)()
        if lib.lp_comm_create_local(world, arr) != OPTIMAL:
            raise LPError(BAD_ARG, "lp_comm_create_local failed")
        return [Comm(_vp(arr[r]), lib) for r in range(world)]

    def rank(self):
        return self.lib.lp_comm_rank(self.h)

    def world(self):
        return self.lib.lp_comm_world(self.h)

    def destroy(self):
        if self.h:
            self.lib.lp_comm_destroy(self.h)
            self.h = None
