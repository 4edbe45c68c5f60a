#!/usr/bin/env python3
"""Device code of two trees, function by function (no GPU needed).

    python scripts/compare_device_code.py --parent REV [--extra=-DFLAG ...] [--out FILE]
    python scripts/compare_device_code.py TREE_A TREE_B [--extra=-DFLAG ...] [--out FILE]

Every simplexmethod_amd/csrc/*.hip of both trees is compiled with build.py's HIPCC_FLAGS (minus -shared) plus
--offload-device-only -S; with --parent REV the first tree is simplexmethod_amd/csrc and include of that revision
(git archive into a temporary directory) and the second is this checkout.  The assembly is split into device functions
by mangled name (a kernel's .amdhsa_* descriptor is part of its text) and the functions are matched across the whole
library, so one may move between files.  Before the comparison .loc, .file, comment and __hip_cuid_* lines are dropped
and the function's index is taken out of its .LBB<n>_<k> and .Lfunc_end<n> labels (it moves with the order of
instantiation).  Prints JSON in the shape of profiles/install_refactor.json; the exit status is 1 if a function differs
or exists on one side only.
"""
import argparse
import difflib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("simplexmethod_amd", "csrc")

_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_SIZE = re.compile(r"^\s*\.size\s+([^\s,]+),")
_DROPPED = re.compile(r"^\s*\.(loc|file)\s")
_LABEL = re.compile(r"\.(LBB|Lfunc_end)\d+")


def normalise(lines):
    """The lines of one function as they are compared."""
    out = []
    for line in lines:
        if _DROPPED.match(line) or "__hip_cuid_" in line:
            continue
        line = line.split(";", 1)[0].rstrip()
        if line:
            out.append(_LABEL.sub(r".\1", line))
    return out


def split_functions(asm):
    """{mangled name: [normalised text, one entry per definition]} of one assembly file's text: a function runs from
    its .type NAME,@function line to its .size NAME line.  (Kernels in anonymous namespaces of two files may share a
    name, hence the list.)"""
    funcs, name, body = {}, None, []
    for line in asm.splitlines():
        if name is None:
            m = _TYPE.match(line)
            if m:
                name, body = m.group(1), []
            continue
        m = _SIZE.match(line)
        if m and m.group(1) == name:
            funcs.setdefault(name, []).append(normalise(body))
            name = None
        else:
            body.append(line)
    return funcs


def merge(per_file):
    """The functions of a whole library from split_functions' results per file."""
    lib = {}
    for funcs in per_file:
        for name, bodies in funcs.items():
            lib.setdefault(name, []).extend(bodies)
    return lib


def differing_lines(a, b):
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def compare(lib_a, lib_b):
    """The report (a dict) of two libraries as merge() returns them."""
    compared, identical, differ, only_a, only_b = 0, 0, {}, [], []
    for name in sorted(set(lib_a) | set(lib_b)):
        a, b = sorted(lib_a.get(name, [])), sorted(lib_b.get(name, []))
        if len(a) != len(b):
            (only_a if len(a) > len(b) else only_b).append(name)
        for x, y in zip(a, b):
            compared += 1
            if x == y:
                identical += 1
            else:
                differ[name] = differ.get(name, 0) + differing_lines(x, y)
    return {"device_functions_compared": compared, "identical": identical, "not_identical": differ,
            "only_in_first": only_a, "only_in_second": only_b}


def compile_tree(root, out_dir, extra):
    """Assembly text of every csrc/*.hip of the tree at root, a few compilers at a time."""
    sys.path.insert(0, ROOT)
    from simplexmethod_amd import build
    flags = [f for f in build.HIPCC_FLAGS if f != "-shared"] + ["--offload-device-only", "-S"] + extra
    csrc = os.path.join(root, CSRC)
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    os.makedirs(out_dir, exist_ok=True)
    hipcc = build.hipcc_path()

    def one(src):
        out = os.path.join(out_dir, src[:-4] + ".s")
        done = subprocess.run([hipcc] + flags + ["-o", out, os.path.join(csrc, src)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)
        if done.returncode:
            raise RuntimeError("%s of %s does not compile:\n%s" % (src, root, done.stdout))
        with open(out) as f:
            return split_functions(f.read())

    with ThreadPoolExecutor(min(6, os.cpu_count() or 1)) as pool:
        return merge(pool.map(one, srcs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("trees", nargs="*", help="two tree roots (instead of --parent)")
    ap.add_argument("--parent", metavar="REV", help="compare this checkout against that revision")
    ap.add_argument("--extra", action="append", default=[], help="a further compiler flag (may be repeated)")
    ap.add_argument("--out", help="write the JSON there as well")
    args = ap.parse_args()
    if bool(args.parent) == bool(args.trees) or (args.trees and len(args.trees) != 2):
        ap.error("give --parent REV or two tree roots")
    with tempfile.TemporaryDirectory() as tmp:
        if args.parent:
            first, second = os.path.join(tmp, "parent"), ROOT
            os.makedirs(first)
            tar = subprocess.run(["git", "-C", ROOT, "archive", args.parent, CSRC, "include"], check=True,
                                 stdout=subprocess.PIPE).stdout
            subprocess.run(["tar", "-x", "-C", first], input=tar, check=True)
        else:
            first, second = args.trees
        report = compare(compile_tree(first, os.path.join(tmp, "asm_a"), args.extra),
                         compile_tree(second, os.path.join(tmp, "asm_b"), args.extra))
    report = {"first": args.parent or first, "second": "this tree" if args.parent else second,
              "extra_flags": args.extra, **report}
    text = json.dumps(report, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if (report["identical"] == report["device_functions_compared"]
                 and not report["only_in_first"] and not report["only_in_second"]) else 1


if __name__ == "__main__":
    sys.exit(main())
