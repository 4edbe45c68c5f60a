"""Builds the in-tree native libraries (hipcc for gfx950, g++ for the host classes).

The built files live under simplexmethod_amd/_build/ (git-ignored, but they travel
to the GPU box with the repo snapshot).  hipcc cross-compiles without a GPU.
"""
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
HOST = os.path.join(_HERE, "host")
OUT = os.path.join(_HERE, "_build")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

HIP_LIB = os.path.join(OUT, "libsimplexmethod_hip.so")
HOST_LIB = os.path.join(OUT, "libsimplexmethod_host.so")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def _newer(target, sources):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(s) <= t for s in sources)


def _sources(d, exts):
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(exts))


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP hot path cannot be built")


def build_hip(force=False, verbose=False):
    """Every csrc/*.hip -> _build/obj/<name>.o (only the stale ones, a few at a time), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OUT, exist_ok=True)
    obj_dir = os.path.join(OUT, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    srcs = _sources(CSRC, (".hip",))
    hdrs = _sources(CSRC, (".hpp",)) + _sources(INCLUDE, (".h",))
    extra = os.environ.get("LP_HIPCC_EXTRA", "").split()
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]
    # the flags are part of an object's identity (LP_HIPCC_EXTRA builds must not reuse plain objects)
    stamp = os.path.join(obj_dir, "flags.txt")
    flag_text = " ".join(flags + extra)
    if not os.path.exists(stamp) or open(stamp).read() != flag_text:
        force = True
    objs, todo = [], []
    for src in srcs:
        obj = os.path.join(obj_dir, os.path.splitext(os.path.basename(src))[0] + ".o")
        objs.append(obj)
        if force or not _newer(obj, [src] + hdrs):
            todo.append((src, obj))
    for stale in set(_sources(obj_dir, (".o",))) - set(objs):
        os.remove(stale)
    if not todo and _newer(HIP_LIB, objs):
        return HIP_LIB
    hipcc = hipcc_path()

    def compile_one(job):
        src, obj = job
        cmd = [hipcc] + flags + extra + ["-c", "-o", obj, src]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    workers = max(1, min(len(todo), int(os.environ.get("LP_BUILD_JOBS", "0")) or min(6, os.cpu_count() or 1)))
    if todo:
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(compile_one, todo))
    with open(stamp, "w") as f:
        f.write(flag_text)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", HIP_LIB] + objs + ["-ldl", "-pthread"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return HIP_LIB


def build_host(force=False, verbose=False):
    """C++ mirror of the reference's problem classes + Solver/EnumerationSolver wrappers."""
    os.makedirs(OUT, exist_ok=True)
    if not os.path.isdir(HOST):
        return None
    srcs = _sources(HOST, (".cpp",))
    if not srcs:
        return None
    deps = srcs + _sources(HOST, (".h",)) + _sources(INCLUDE, (".h",))
    if not force and _newer(HOST_LIB, deps):
        return HOST_LIB
    build_hip(force=False, verbose=verbose)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", INCLUDE,
           "-I", HOST, "-o", HOST_LIB] + srcs + ["-L", OUT, "-lsimplexmethod_hip",
                                                  "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return HOST_LIB


TESTS_CPP = os.path.join(os.path.dirname(_HERE), "tests", "cpp")
TESTS_OUT = os.path.join(TESTS_CPP, "_build")


def build_cpp_tests(force=False, verbose=False):
    """tests/cpp/*.cpp -> tests/cpp/_build/<name> (linked against the host + HIP libraries)."""
    host = build_host(force, verbose)
    if host is None or not os.path.isdir(TESTS_CPP):
        return []
    os.makedirs(TESTS_OUT, exist_ok=True)
    outs = []
    for src in _sources(TESTS_CPP, (".cpp",)):
        exe = os.path.join(TESTS_OUT, os.path.splitext(os.path.basename(src))[0])
        deps = [src, host, HIP_LIB] + _sources(TESTS_CPP, (".h",)) + _sources(HOST, (".h",))
        if force or not _newer(exe, deps):
            cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-DLP_HOST_TEST_HOOKS", "-I", INCLUDE, "-I", HOST, "-I", TESTS_CPP,
                   "-o", exe, src, "-L", OUT, "-lsimplexmethod_host", "-lsimplexmethod_hip",
                   "-pthread", "-Wl,-rpath,$ORIGIN/../../../simplexmethod_amd/_build"]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
        outs.append(exe)
    return outs


TESTS_REF = os.path.join(os.path.dirname(_HERE), "tests", "ref")
TEST_REF_LIB = os.path.join(TESTS_REF, "_build", "libbland_ref.so")


def build_test_ref(force=False, verbose=False):
    """tests/ref/bland_ref.c -> tests/ref/_build/libbland_ref.so: the pivot-rule restatement the tests
    compare against (plain C, no GPU; fused multiply-adds only where the source writes fma())."""
    src = os.path.join(TESTS_REF, "bland_ref.c")
    if not os.path.exists(src):
        return None
    if not force and _newer(TEST_REF_LIB, [src]):
        return TEST_REF_LIB
    os.makedirs(os.path.dirname(TEST_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", TEST_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return TEST_REF_LIB


DEVEX_REF_LIB = os.path.join(TESTS_REF, "_build", "libdevex_ref.so")


def build_test_devex_ref(force=False, verbose=False):
    """tests/ref/devex_ref.c -> tests/ref/_build/libdevex_ref.so: the Devex restatement the tests compare
    against; flags as build_test_ref."""
    src = os.path.join(TESTS_REF, "devex_ref.c")
    if not os.path.exists(src):
        return None
    if not force and _newer(DEVEX_REF_LIB, [src]):
        return DEVEX_REF_LIB
    os.makedirs(os.path.dirname(DEVEX_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", DEVEX_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return DEVEX_REF_LIB


RESOLVE_REF_LIB = os.path.join(TESTS_REF, "_build", "libresolve_ref.so")


def build_resolve_ref(force=False, verbose=False):
    """tests/ref/resolve_ref.c -> tests/ref/_build/libresolve_ref.so: the re-solve from a given basis
    (primal or dual simplex) the tests compare against; flags as build_test_ref."""
    src = os.path.join(TESTS_REF, "resolve_ref.c")
    if not os.path.exists(src):
        return None
    if not force and _newer(RESOLVE_REF_LIB, [src]):
        return RESOLVE_REF_LIB
    os.makedirs(os.path.dirname(RESOLVE_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", RESOLVE_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return RESOLVE_REF_LIB


DUALS_REF_LIB = os.path.join(TESTS_REF, "_build", "libduals_ref.so")


def build_duals_ref(force=False, verbose=False):
    """tests/ref/duals_ref.c -> tests/ref/_build/libduals_ref.so: the dual solution at a given basis the
    tests compare against; flags as build_test_ref."""
    src = os.path.join(TESTS_REF, "duals_ref.c")
    if not os.path.exists(src):
        return None
    if not force and _newer(DUALS_REF_LIB, [src]):
        return DUALS_REF_LIB
    os.makedirs(os.path.dirname(DUALS_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", DUALS_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return DUALS_REF_LIB


RANGING_REF_LIB = os.path.join(TESTS_REF, "_build", "libranging_ref.so")


def build_ranging_ref(force=False, verbose=False):
    """tests/ref/ranging_ref.c (which includes duals_ref.c) -> tests/ref/_build/libranging_ref.so: RHS and cost
    ranging at a given basis the tests compare against; flags as build_duals_ref."""
    src = os.path.join(TESTS_REF, "ranging_ref.c")
    if not os.path.exists(src):
        return None
    if not force and _newer(RANGING_REF_LIB, [src, os.path.join(TESTS_REF, "duals_ref.c")]):
        return RANGING_REF_LIB
    os.makedirs(os.path.dirname(RANGING_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", RANGING_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return RANGING_REF_LIB


CERTIFICATE_REF_LIB = os.path.join(TESTS_REF, "_build", "libcertificate_ref.so")


def build_certificate_ref(force=False, verbose=False):
    """tests/ref/certificate_ref.c (which includes ranging_ref.c and duals_ref.c) ->
    tests/ref/_build/libcertificate_ref.so: Farkas and ray certificates at a given basis the tests compare against;
    flags as build_ranging_ref."""
    src = os.path.join(TESTS_REF, "certificate_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(TESTS_REF, "ranging_ref.c"), os.path.join(TESTS_REF, "duals_ref.c")]
    if not force and _newer(CERTIFICATE_REF_LIB, deps):
        return CERTIFICATE_REF_LIB
    os.makedirs(os.path.dirname(CERTIFICATE_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", CERTIFICATE_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return CERTIFICATE_REF_LIB


PARAMETRIC_REF_LIB = os.path.join(TESTS_REF, "_build", "libparametric_ref.so")


def build_parametric_ref(force=False, verbose=False):
    """tests/ref/parametric_ref.c (which includes resolve_ref.c) -> tests/ref/_build/libparametric_ref.so: the
    parametric right-hand-side path from an optimal basis the tests compare against; flags as build_resolve_ref."""
    src = os.path.join(TESTS_REF, "parametric_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(TESTS_REF, "resolve_ref.c")]
    if not force and _newer(PARAMETRIC_REF_LIB, deps):
        return PARAMETRIC_REF_LIB
    os.makedirs(os.path.dirname(PARAMETRIC_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", PARAMETRIC_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return PARAMETRIC_REF_LIB


PARAMETRIC_COST_REF_LIB = os.path.join(TESTS_REF, "_build", "libparametric_cost_ref.so")


def build_parametric_cost_ref(force=False, verbose=False):
    """tests/ref/parametric_cost_ref.c (which includes resolve_ref.c) -> tests/ref/_build/libparametric_cost_ref.so:
    the parametric cost path from an optimal basis the tests compare against; flags as build_resolve_ref."""
    src = os.path.join(TESTS_REF, "parametric_cost_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(TESTS_REF, "resolve_ref.c")]
    if not force and _newer(PARAMETRIC_COST_REF_LIB, deps):
        return PARAMETRIC_COST_REF_LIB
    os.makedirs(os.path.dirname(PARAMETRIC_COST_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", PARAMETRIC_COST_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return PARAMETRIC_COST_REF_LIB


MIP_REF_LIB = os.path.join(TESTS_REF, "_build", "libmip_ref.so")


def build_mip_ref(force=False, verbose=False):
    """tests/ref/mip_ref.c (which includes resolve_ref.c) -> tests/ref/_build/libmip_ref.so: the depth-first
    branch-and-bound the tests compare against; flags as build_resolve_ref."""
    src = os.path.join(TESTS_REF, "mip_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(TESTS_REF, "resolve_ref.c")]
    if not force and _newer(MIP_REF_LIB, deps):
        return MIP_REF_LIB
    os.makedirs(os.path.dirname(MIP_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", MIP_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return MIP_REF_LIB


BOUNDED_REF_LIB = os.path.join(TESTS_REF, "_build", "libbounded_ref.so")


def build_bounded_ref(force=False, verbose=False):
    """tests/ref/bounded_ref.c -> tests/ref/_build/libbounded_ref.so: the two-phase bounded-variable simplex the tests
    compare against; flags as build_test_ref."""
    src = os.path.join(TESTS_REF, "bounded_ref.c")
    if not os.path.exists(src):
        return None
    if not force and _newer(BOUNDED_REF_LIB, [src]):
        return BOUNDED_REF_LIB
    os.makedirs(os.path.dirname(BOUNDED_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", BOUNDED_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return BOUNDED_REF_LIB


BOUNDED_RESOLVE_REF_LIB = os.path.join(TESTS_REF, "_build", "libbounded_resolve_ref.so")


def build_bounded_resolve_ref(force=False, verbose=False):
    """tests/ref/bounded_resolve_ref.c (which includes bounded_ref.c) -> tests/ref/_build/libbounded_resolve_ref.so:
    the bounded-variable re-solve from a given basis the tests compare against; flags as build_bounded_ref."""
    src = os.path.join(TESTS_REF, "bounded_resolve_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(TESTS_REF, "bounded_ref.c")]
    if not force and _newer(BOUNDED_RESOLVE_REF_LIB, deps):
        return BOUNDED_RESOLVE_REF_LIB
    os.makedirs(os.path.dirname(BOUNDED_RESOLVE_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", BOUNDED_RESOLVE_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return BOUNDED_RESOLVE_REF_LIB


MIP_BOUNDED_REF_LIB = os.path.join(TESTS_REF, "_build", "libmip_bounded_ref.so")


def build_mip_bounded_ref(force=False, verbose=False):
    """tests/ref/mip_bounded_ref.c (which includes bounded_resolve_ref.c and bounded_ref.c) ->
    tests/ref/_build/libmip_bounded_ref.so: the branch-and-bound over variable bounds the tests compare against; flags
    as build_bounded_resolve_ref."""
    src = os.path.join(TESTS_REF, "mip_bounded_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(TESTS_REF, "bounded_resolve_ref.c"), os.path.join(TESTS_REF, "bounded_ref.c")]
    if not force and _newer(MIP_BOUNDED_REF_LIB, deps):
        return MIP_BOUNDED_REF_LIB
    os.makedirs(os.path.dirname(MIP_BOUNDED_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", MIP_BOUNDED_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return MIP_BOUNDED_REF_LIB


BOUNDED_SENS_REF_LIB = os.path.join(TESTS_REF, "_build", "libbounded_sens_ref.so")


def build_bounded_sens_ref(force=False, verbose=False):
    """tests/ref/bounded_sens_ref.c (which includes ranging_ref.c and duals_ref.c) ->
    tests/ref/_build/libbounded_sens_ref.so: the dual solution and ranging of a bounded-variable LP at a given basis
    and flags the tests compare against; flags as build_ranging_ref."""
    src = os.path.join(TESTS_REF, "bounded_sens_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(TESTS_REF, "ranging_ref.c"), os.path.join(TESTS_REF, "duals_ref.c")]
    if not force and _newer(BOUNDED_SENS_REF_LIB, deps):
        return BOUNDED_SENS_REF_LIB
    os.makedirs(os.path.dirname(BOUNDED_SENS_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", BOUNDED_SENS_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return BOUNDED_SENS_REF_LIB


BOUNDED_CERTIFICATE_REF_LIB = os.path.join(TESTS_REF, "_build", "libbounded_certificate_ref.so")


def build_bounded_certificate_ref(force=False, verbose=False):
    """tests/ref/bounded_certificate_ref.c (which includes certificate_ref.c, ranging_ref.c and duals_ref.c) ->
    tests/ref/_build/libbounded_certificate_ref.so: Farkas and ray certificates of a bounded-variable LP at a given
    basis and flags the tests compare against; flags as build_certificate_ref."""
    src = os.path.join(TESTS_REF, "bounded_certificate_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src] + [os.path.join(TESTS_REF, f) for f in ("certificate_ref.c", "ranging_ref.c", "duals_ref.c")]
    if not force and _newer(BOUNDED_CERTIFICATE_REF_LIB, deps):
        return BOUNDED_CERTIFICATE_REF_LIB
    os.makedirs(os.path.dirname(BOUNDED_CERTIFICATE_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", BOUNDED_CERTIFICATE_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return BOUNDED_CERTIFICATE_REF_LIB


BOUNDED_PARAMETRIC_REF_LIB = os.path.join(TESTS_REF, "_build", "libbounded_parametric_ref.so")


def build_bounded_parametric_ref(force=False, verbose=False):
    """tests/ref/bounded_parametric_ref.c (which includes bounded_resolve_ref.c and bounded_ref.c) ->
    tests/ref/_build/libbounded_parametric_ref.so: the parametric right-hand-side and cost paths of a bounded-variable
    LP from an optimal basis and flags the tests compare against; flags as build_bounded_resolve_ref."""
    src = os.path.join(TESTS_REF, "bounded_parametric_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src] + [os.path.join(TESTS_REF, f) for f in ("bounded_resolve_ref.c", "bounded_ref.c")]
    if not force and _newer(BOUNDED_PARAMETRIC_REF_LIB, deps):
        return BOUNDED_PARAMETRIC_REF_LIB
    os.makedirs(os.path.dirname(BOUNDED_PARAMETRIC_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", BOUNDED_PARAMETRIC_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return BOUNDED_PARAMETRIC_REF_LIB


BOUNDED_RULES_REF_LIB = os.path.join(TESTS_REF, "_build", "libbounded_rules_ref.so")


def build_bounded_rules_ref(force=False, verbose=False):
    """tests/ref/bounded_rules_ref.c (which includes bounded_ref.c) -> tests/ref/_build/libbounded_rules_ref.so: the
    two-phase bounded-variable simplex under Dantzig's, Bland's or the Devex rule the tests compare against; flags as
    build_bounded_ref."""
    src = os.path.join(TESTS_REF, "bounded_rules_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(TESTS_REF, "bounded_ref.c")]
    if not force and _newer(BOUNDED_RULES_REF_LIB, deps):
        return BOUNDED_RULES_REF_LIB
    os.makedirs(os.path.dirname(BOUNDED_RULES_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", BOUNDED_RULES_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return BOUNDED_RULES_REF_LIB


BOUNDED_RESOLVE_RULES_REF_LIB = os.path.join(TESTS_REF, "_build", "libbounded_resolve_rules_ref.so")


def build_bounded_resolve_rules_ref(force=False, verbose=False):
    """tests/ref/bounded_resolve_rules_ref.c (which includes bounded_resolve_ref.c, bounded_ref.c and
    bounded_rules_ref.c) -> tests/ref/_build/libbounded_resolve_rules_ref.so: the bounded-variable re-solve whose primal
    branch runs under a pivot rule; flags as build_bounded_ref."""
    src = os.path.join(TESTS_REF, "bounded_resolve_rules_ref.c")
    if not os.path.exists(src):
        return None
    deps = [src] + [os.path.join(TESTS_REF, f) for f in ("bounded_rules_ref.c", "bounded_resolve_ref.c", "bounded_ref.c")]
    if not force and _newer(BOUNDED_RESOLVE_RULES_REF_LIB, deps):
        return BOUNDED_RESOLVE_RULES_REF_LIB
    os.makedirs(os.path.dirname(BOUNDED_RESOLVE_RULES_REF_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-Wall", "-Wextra",
           "-o", BOUNDED_RESOLVE_RULES_REF_LIB, src, "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return BOUNDED_RESOLVE_RULES_REF_LIB


def build_all(force=False, verbose=False):
    hip, host = build_hip(force, verbose), build_host(force, verbose)
    build_cpp_tests(force, verbose)
    build_test_ref(force, verbose)
    build_test_devex_ref(force, verbose)
    build_resolve_ref(force, verbose)
    build_duals_ref(force, verbose)
    build_ranging_ref(force, verbose)
    build_certificate_ref(force, verbose)
    build_parametric_ref(force, verbose)
    build_parametric_cost_ref(force, verbose)
    build_mip_ref(force, verbose)
    build_bounded_ref(force, verbose)
    build_bounded_resolve_ref(force, verbose)
    build_mip_bounded_ref(force, verbose)
    build_bounded_sens_ref(force, verbose)
    build_bounded_certificate_ref(force, verbose)
    build_bounded_parametric_ref(force, verbose)
    build_bounded_rules_ref(force, verbose)
    build_bounded_resolve_rules_ref(force, verbose)
    return hip, host


if __name__ == "__main__":
    import sys
    print(build_all(force="--force" in sys.argv, verbose=True))
