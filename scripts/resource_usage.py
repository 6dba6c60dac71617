#!/usr/bin/env python3
"""Register table of the engine's kernels, from the compiler's own report.

Compiles the device code of csrc/unetpp_abi.hip with the library's flags (unet_amd._lib.CXXFLAGS) plus
-Rpass-analysis=kernel-resource-usage into a temporary directory and parses the remarks -- nothing else: the
assembly is not searched.  No GPU needed.

usage: python scripts/resource_usage.py [--all] [--remarks FILE] [--save-remarks FILE] [pattern ...]
  pattern       substrings of the demangled kernel name (default: conv3x3_ws and tapmm_ws_kernel)
  --all         every kernel of the translation unit
  --remarks     parse a saved compiler log instead of compiling
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
          "LDS Size [bytes/block]": "lds"}
_REMARK = re.compile(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]")


def compile_remarks(defines=()) -> str:
    """The compiler's log of a device-only compile of unetpp_abi.hip with the product flags."""
    from unet_amd import _lib
    hipcc = _lib._hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory(prefix="unetpp_ru_") as tmp:
        cmd = [hipcc] + _lib.CXXFLAGS + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                         '-DUNETPP_SRC_HASH="resource-usage"'] + [f"-D{d}" for d in defines] + [
               "-o", os.path.join(tmp, "unetpp_abi.o"), os.path.join(_lib.CSRC, "unetpp_abi.hip")]
        r = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("compile failed:\n" + r.stdout[-4000:])
        return r.stdout


def _demangle_simple(name: str) -> str:
    """_ZN6unetpp<len><kernel>I<Li2E|Lb0E ...>EEv... -> kernel<2, false, ...> (integer and bool template arguments only)"""
    m = re.match(r"_ZN6unetpp(\d+)", name)
    if not m:
        return name
    n = int(m.group(1))
    base, rest = name[m.end():m.end() + n], name[m.end() + n:]
    t = re.match(r"I((?:L[ib]n?\d+E)+)E", rest)
    if not t:
        return base
    args = [("true" if v != "0" else "false") if k == "b" else v.replace("n", "-") for k, v in re.findall(r"L([ib])(n?\d+)E", t.group(1))]
    return f"{base}<{', '.join(args)}>"


def demangle(names):
    """Mangled -> demangled kernel names (llvm-cxxfilt or c++filt; the mangled name where neither is at hand)."""
    tool = None
    for cand in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if cand and os.path.exists(cand):
            tool = cand
            break
    if not tool or not names:
        return {n: _demangle_simple(n) for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"^void |\(unetpp::ConvArgs\)$|\(.*\)$|unetpp::", "", d) for n, d in zip(names, out)}


def parse_remarks(log: str) -> dict:
    """{demangled kernel name: {sgprs, vgprs, agprs, scratch, occupancy, sgpr_spill, vgpr_spill, lds}}"""
    raw, cur = {}, None
    for line in log.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = raw.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    names = demangle(list(raw))
    return {names[k]: v for k, v in raw.items()}


def short(name: str) -> str:
    """conv3x3_ws_kernel<2, true, false, ...> -> conv3x3_ws_kernel<2,T,F,...>"""
    return name.replace("true", "T").replace("false", "F").replace(", ", ",")


def table(kernels: dict, patterns) -> str:
    rows = [f"{'kernel':64s} {'SGPRs':>5s} {'VGPRs':>5s} {'AGPRs':>5s} {'sSpill':>6s} {'vSpill':>6s} {'scratch':>7s} {'occ':>3s}"]
    for name in sorted(kernels):
        if patterns and not any(p in name for p in patterns):
            continue
        k = kernels[name]
        rows.append(f"{short(name):64s} {k.get('sgprs', -1):5d} {k.get('vgprs', -1):5d} {k.get('agprs', -1):5d} "
                    f"{k.get('sgpr_spill', -1):6d} {k.get('vgpr_spill', -1):6d} {k.get('scratch', -1):7d} {k.get('occupancy', -1):3d}")
    return "\n".join(rows)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("patterns", nargs="*")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--remarks")
    ap.add_argument("--save-remarks")
    args = ap.parse_args()
    if args.remarks:
        with open(args.remarks) as f:
            log = f.read()
    else:
        log = compile_remarks()
    if args.save_remarks:
        with open(args.save_remarks, "w") as f:
            f.write(log)
    patterns = [] if args.all else (args.patterns or ["conv3x3_ws", "tapmm_ws_kernel"])
    print(table(parse_remarks(log), patterns))


if __name__ == "__main__":
    main()
