#!/usr/bin/env python3
"""The optimiser step on the device (unet_amd/optim.py) against the same update by torch, on the parameter sets of the 3-class
deep-supervision NestedUNet and of SimpleUNet (shapes from synthetic.make_state_dict / make_simple_state_dict; every float
weight and bias, the BatchNorm statistics excluded).  clip_grad_norm_(max_norm=1) + AdamW, gradients already in place.

Device events around `--iters` calls after `--warmup` calls, three loops; every time is the median with the fastest and the
slowest loop beside it (microseconds).  Per workload, without and with a loss scaler (suffix _scaler):
  norm_launch_us, step_launch_us   unetpp_optim_grad_norm_f32 / unetpp_optim_step_f32 alone (the C entries, fixed arguments)
  both_launches_us                 the two entries back to back
  step_us, step_wall_us            optim.AdamW.step() from Python: device time, and host clock per call between two synchronisations
  torch_default_us                 clip_grad_norm_ + torch.optim.AdamW (its default, the multi-tensor form), GradScaler.unscale_/step/update
  torch_fused_us                   the same with fused=True
  bytes_norm = 4 n, bytes_step = 28 n (32 n with zero_grads): g read | g, p, m, v read and p, m, v written
  norm_share_of_hbm, step_share_of_hbm   bytes over launch time, as a fraction of 6.3 TB/s
The parameters after one step are compared between the routes before anything is timed.

    python scripts/optim_bench.py [--iters 200] [--warmup 5] [--out OUT.txt]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_timing import timed_spread, wall  # noqa: E402
HBM_BYTES_PER_US = 6.3e6                                        # 6.3 TB/s
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def workloads():
    from unet_amd import synthetic
    sets = {"nested_3class_ds": synthetic.make_state_dict(3, 3, True, 0), "simple_7class": synthetic.make_simple_state_dict(7, 3, 0)}
    return {name: [v for k, v in sd.items() if v.dtype == np.float32 and k.split(".")[-1] in ("weight", "bias")] for name, sd in sets.items()}


def bench(torch, name, arrays, iters, warmup):
    from unet_amd import _lib_optim, optim
    dev = "cuda"
    rng = np.random.default_rng(0)
    grads = [(rng.standard_normal(a.shape) * 1e-2).astype(np.float32) for a in arrays]

    def fresh():
        params = [torch.nn.Parameter(torch.from_numpy(a).to(dev)) for a in arrays]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g).to(dev)
        return params

    ours = fresh()
    opt = optim.AdamW(ours, max_norm=1.0, **HYPER)
    a = opt.arena
    row = {"workload": name, "tensors": len(arrays), "n": a.n, "elements": int(sum(x.size for x in arrays)), "chunk": optim.chunk_for(a.n),
           "workgroups": optim.parts_for(a.n), "bytes_norm": 4 * a.n, "bytes_step": 28 * a.n}

    # one step by each route on the same input: the routes must agree before they are timed
    theirs = fresh()
    topt = torch.optim.AdamW(theirs, **HYPER)
    torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    topt.step()
    opt.step()
    torch.cuda.synchronize()
    diff = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(ours, theirs))
    row["max_diff_after_one_step"] = diff
    assert diff < 1e-6, diff

    lib = _lib_optim.load()
    G, A = opt._fill_groups(), _lib_optim.StepArgs()
    A.use_clip, A.max_norm, A.growth_factor, A.backoff_factor, A.growth_interval = 1, 1.0, 2.0, 0.5, 2000
    ws, st = opt._workspace.data_ptr(), torch.zeros(2 * optim.SLOT_WORDS, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    scaler = optim.LossScaler(dev, init_scale=1.0)                # scale 1: the gradients stay as they are

    def norm():
        assert lib.unetpp_optim_grad_norm_f32(a.grad.data_ptr(), a.n, ws, stream) == 0

    def step(sc=None):
        assert lib.unetpp_optim_step_f32(a.flat.data_ptr(), a.grad.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), a.n, ctypes.byref(G), ctypes.byref(A),
                                         ws, st.data_ptr(), sc, stream) == 0

    def both(sc=None):
        norm()
        step(sc)

    for suffix, sc, scaler_obj in (("", None, None), ("_scaler", scaler._state.data_ptr(), scaler)):
        row["norm_launch_us"] = timed_spread(torch, norm, iters, warmup)
        row["step_launch_us" + suffix] = timed_spread(torch, lambda: step(sc), iters, warmup)
        row["both_launches_us" + suffix] = timed_spread(torch, lambda: both(sc), iters, warmup)
        row["step_us" + suffix] = timed_spread(torch, lambda: opt.step(scaler=scaler_obj), iters, warmup)
        row["step_wall_us" + suffix] = wall(torch, lambda: opt.step(scaler=scaler_obj), iters, warmup)
        row["step_share_of_hbm" + suffix] = round(row["bytes_step"] / row["step_launch_us" + suffix][0] / HBM_BYTES_PER_US, 3)
    row["norm_share_of_hbm"] = round(row["bytes_norm"] / row["norm_launch_us"][0] / HBM_BYTES_PER_US, 3)

    for label, kw in (("torch_default_us", {}), ("torch_fused_us", {"fused": True})):
        params = fresh()
        topt = torch.optim.AdamW(params, **HYPER, **kw)

        def plain():
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            topt.step()
        row[label] = timed_spread(torch, plain, iters, warmup)
        gs = torch.amp.GradScaler("cuda", init_scale=1.0)
        gs.scale(torch.zeros((), device=dev))

        def scaled():
            gs.unscale_(topt)
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            gs.step(topt)
            gs.update()
        row[label.replace("_us", "_scaler_us")] = timed_spread(torch, scaled, iters, warmup)
    for suffix in ("", "_scaler"):
        row["torch_fused_over_step" + suffix] = round(row["torch_fused" + suffix + "_us"][0] / row["step_us" + suffix][0], 2)
        row["torch_default_over_step" + suffix] = round(row["torch_default" + suffix + "_us"][0] / row["step_us" + suffix][0], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from unet_amd import _lib_optim
    assert torch.cuda.is_available(), "optim_bench.py needs a HIP device; there is nothing to measure without one"
    lines = [_lib_optim.load().unetpp_optim_version().decode()]
    for name, arrays in workloads().items():
        lines.append(json.dumps(bench(torch, name, arrays, args.iters, args.warmup)))
        print(lines[-1], flush=True)
    lines.append(json.dumps({"training_step_with_the_network": "not measured"}))
    out = args.out or os.path.join(ROOT, "profiles", f"optim_{_lib_optim.source_hash()}_bench.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
