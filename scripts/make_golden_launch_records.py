#!/usr/bin/env python3
"""Record tests/golden/launch_records.json: label, flops, bytes and plan of every launch of the configurations of
tests/test_gpu_launch_records.py (its CASES, each planned for 8 and for 64 compute units), through the public Python API.

    python scripts/make_golden_launch_records.py --commit <hash> [--tree DIR] [--out FILE]

Runs on the MI355X.  --tree DIR records the engine of another checkout of this repository (its unet_amd package and the library
built in it) instead of this one: the fixture in git was recorded that way from the commit its README names, before the host
code of unetpp_abi.hip was taken apart, and is what the taken-apart code is held to.  Record again only when a launch is MEANT
to change, and say in the README from which commit."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="checkout whose engine is recorded (default: this one)")
    ap.add_argument("--commit", required=True, help="the commit of that checkout, written into the fixture")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_records.json"))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import unet_amd                      # before the test modules: their conftest puts this checkout first on sys.path
    assert os.path.dirname(unet_amd.__path__[0]) == tree, unet_amd.__path__
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import test_gpu_launch_records as t
    from unet_amd import _lib, synthetic
    records = {}
    for key in t.CASES:
        for n in t.PLAN_CUS:
            records[f"{key} cus={n}"] = t.record_case(torch, synthetic, key, n)
            print(f"{key} cus={n}: " + ", ".join(f"{name}: {len(r)} launches" for name, r in records[f"{key} cus={n}"].items()), flush=True)
    doc = {"commit": args.commit, "library": _lib.load().unetpp_version().decode(), "plan_cus": list(t.PLAN_CUS),
           "record": ["label", "flops", "bytes", "grid", "tiles", "ksplit", "rows"], "records": records}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {sum(len(r) for c in records.values() for r in c.values())} records")


if __name__ == "__main__":
    main()
