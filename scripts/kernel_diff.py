#!/usr/bin/env python3
"""Are the engine's kernels of two source trees instruction-identical?  The check a refactor of the kernels is held to.

Compiles the device code of csrc/unetpp_abi.hip of each tree with the library's flags (unet_amd._lib.CXXFLAGS) plus
--cuda-device-only -S into a temporary directory and compares, per kernel, the text between its label and its
.Lfunc_end (comments stripped) together with its .amdhsa_* directives, and the amdhsa.kernels metadata of the whole
file.  Text is compared, nothing is searched for; the __hip_cuid_* symbol (a hash of the source) lies outside all of
these.  No GPU needed.  Exit status 1 on any difference.

usage: python scripts/kernel_diff.py [--against COMMIT | --a DIR] [--b DIR] [-DNAME[=VALUE] ...]
  --against  the other tree is a git worktree of COMMIT under build/ (default HEAD); --a names a directory instead
  --b        the tree under test (default: the working tree)
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def device_asm(tree: str, defines, out: str) -> str:
    from unet_amd import _lib
    cmd = [_lib._hipcc()] + _lib.CXXFLAGS + ["--cuda-device-only", "-S", '-DUNETPP_SRC_HASH="kernel-diff"'] + [
        f"-D{d}" for d in defines] + ["-o", out, os.path.join(tree, os.path.relpath(_lib.CSRC, ROOT), "unetpp_abi.hip")]
    r = subprocess.run(cmd, cwd=os.path.dirname(out), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise SystemExit(f"compile of {tree} failed:\n{r.stdout[-4000:]}")
    with open(out) as f:
        return f.read()


def kernels(asm: str) -> dict:
    """{kernel symbol: its instructions and .amdhsa_* directives, comments stripped}, plus the metadata under '(metadata)'"""
    lines = [s for s in (re.sub(r"\s*;.*", "", line).strip() for line in asm.splitlines()) if s]
    out = {}
    for i, line in enumerate(lines):
        if line.startswith(".amdhsa_kernel "):
            name = line.split()[1]
            body = lines[lines.index(name + ":"):]
            body = body[:next(j for j, s in enumerate(body) if s.startswith(".Lfunc_end"))]
            out[name] = body + lines[i:lines.index(".end_amdhsa_kernel", i)]
    out["(metadata)"] = lines[lines.index(".amdgpu_metadata"):lines.index(".end_amdgpu_metadata")]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--against", default="HEAD")
    ap.add_argument("--a")
    ap.add_argument("--b", default=ROOT)
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--keep", help="an existing directory in which a.s and b.s are left, to look at a difference")
    args = ap.parse_args()
    a = args.a
    if not a:
        rev = subprocess.run(["git", "rev-parse", "--short", args.against], cwd=ROOT, stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
        a = os.path.join(ROOT, "build", "kernel_diff", rev)
        if not os.path.isdir(a):
            subprocess.run(["git", "worktree", "add", "--detach", a, rev], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory(prefix="unetpp_kd_") as tmp, ThreadPoolExecutor(2) as ex:
        tmp = args.keep or tmp
        ka, kb = ex.map(lambda t: kernels(device_asm(t[1], args.defines, os.path.join(tmp, t[0] + ".s"))), (("a", a), ("b", args.b)))
    same = 0
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print(f"{'added' if name in kb else 'removed'}: {name}")
        elif ka[name] != kb[name]:
            n = sum(1 for d in difflib.unified_diff(ka[name], kb[name], n=0, lineterm="") if d[0] in "+-" and d[:3] not in ("+++", "---"))
            print(f"differs ({n} lines): {name}")
        else:
            same += 1
    total = len(set(ka) | set(kb)) - 1
    n_same = same - (ka["(metadata)"] == kb["(metadata)"])
    print(f"{n_same} of {total} kernels identical; metadata {'identical' if ka['(metadata)'] == kb['(metadata)'] else 'differs'}"
          f"{' [' + ' '.join('-D' + d for d in args.defines) + ']' if args.defines else ''}")
    return 0 if same == total + 1 else 1


if __name__ == "__main__":
    sys.exit(main())
