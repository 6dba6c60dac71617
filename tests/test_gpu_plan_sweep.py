"""The persistent tile walk at small shapes: engines planned for fewer compute units than the device has (UNETPP_PLAN_CUS=n,
include/unetpp.h), so that a workgroup of conv3x3_ws_kernel and its split-K and low-row siblings, of conv3x3_bias_relu_kernel
and of tapmm_ws_kernel walks several tiles at shapes small enough to compare every stored plane of every node.

a. the walk changes no bit: every output and every stored plane of an engine planned for n CUs equals the same engine planned
   for the device (one tile per workgroup: none of the inter-tile code runs), and that baseline is held to the CPU oracle over
   all pixels at its mode's existing bar;
b. the coverage is asserted from the launches' own plan report (unetpp_profile_plan), not from reasoning;
c. split-K under other plans, d. split-K on concurrent internal streams.

tests/test_plan_host.py pins the tile-number stepping as an algorithm; this file pins the kernels.
Run on the GPU box:  python -m pytest tests -m gpu"""
import contextlib
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_exact8 import gate
from test_gpu_parity import NODES, report

pytestmark = pytest.mark.gpu

N_PLANS = (1, 2, 3, 5, 7, 8, 16, 24)
SIMPLE_NODES = ("enc1", "enc2", "enc3", "enc4", "up3t", "dec3", "up2t", "dec2", "up1t", "dec1")
NB = (32, 64, 128, 256, 512)
SB = (64, 128, 256, 512)
PLAN_ENV = ("UNETPP_PLAN_CUS", "UNETPP_KSPLIT", "UNETPP_TAPMM", "UNETPP_UPROWS")

# name -> (arch, classes, batch, H, W, precision, extra switches)
S1, S2, SU = (7, 3, 48, 80), (3, 2, 80, 112), (7, 2, 40, 72)
CONFIGS = {
    "S1-exact": ("nested", *S1, "exact", {}), "S1-exact8": ("nested", *S1, "exact8", {}), "S1-fast": ("nested", *S1, "fast", {}),
    "S2-exact": ("nested", *S2, "exact", {}), "S2-exact8": ("nested", *S2, "exact8", {}), "S2-fast": ("nested", *S2, "fast", {}),
    "simple-exact": ("simple", *SU, "exact", {}), "simple-exact8": ("simple", *SU, "exact8", {}),
    "S1-exact-tapmm-none": ("nested", *S1, "exact", {"UNETPP_TAPMM": "none"}),
    "S1-exact-tapmm-3": ("nested", *S1, "exact", {"UNETPP_TAPMM": "3"}),
    "S1-exact-uprows-none": ("nested", *S1, "exact", {"UNETPP_UPROWS": "none"}),
    "S3-fast": ("nested", 3, 6, 48, 80, "fast", {}),
}
# "For n <= 5 every persistent launch has more tiles than workgroups" does not hold at S1 and S2 for fast mode's level 2 (and one
# pooled level-3 conv): there the lock-step kernel's tile is 128 channels wide, Cout = 128 is ONE channel tile, and a 12 x 20 or
# 20 x 28 level has one or two pixel tiles per image -- 3 resp. 4 tiles in all, no more than n = 3 or 5 (measured from the plan
# report).  They are named here and held to exactly this set; S3 (the S1 frame size at batch 6, the smallest batch with more than
# five tiles in every launch) makes the same launches walk at every n <= 5, with nothing excepted.
ONE_TILE_PER_IMAGE = {
    ("S1-fast", 3): {"conv2_0.conv1", "conv2_0.conv2", "conv2_2.conv1", "conv2_2.conv2"},
    ("S1-fast", 5): {"conv2_0.conv2"},
    ("S2-fast", 5): {"conv2_0.conv2", "conv3_0.conv2"},
}
FAMILIES = ("plain", "pool", "head", "up 1x4", "up 2x2", "low-row", "first block", "two-source", "lock-step", "gemm")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@contextlib.contextmanager
def plan_env(**switches):
    """The plan switches unetpp_create reads, set for the creation of one engine and put back afterwards."""
    old = {k: os.environ.get(k) for k in PLAN_ENV}
    for k in PLAN_ENV:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in switches.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def device_cus(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def make_engine(torch, arch, C, sd, B, hw, precision, x, switches, **kw):
    """An engine created under `switches` (the first forward creates it); the switches are gone again when this returns."""
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    if arch == "nested":
        m = NestedUNet(C, deep_supervision=False, precision=precision, max_batch=B, max_hw=hw, **kw).to("cuda:0")
    else:
        m = SimpleUNet(num_classes=C, num_channels=3, precision=precision, max_batch=B, max_hw=hw, **kw).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    m.eval()
    with plan_env(**switches):
        m(x)
    torch.cuda.synchronize()
    return m


def planes_of(precision):
    """the stored planes of a node as unetpp_debug_read names them; fast stores one fp16 plane: the node itself"""
    return {"exact": ("#hi", "#lo"), "exact8": ("#hi", "#lo", "#x8"), "fast": ("",)}[precision]


def read_plane(model, name, shape):
    from unet_amd import _lib
    out = np.empty(shape, dtype=np.float32)
    n = _lib.load().unetpp_debug_read(model._handle, name.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
    assert n == out.size, (name, n, model._err(int(n)) if n < 0 else out.size)
    return out


def node_shape(arch, name, B, H, W):
    if arch == "nested":
        lvl = int(name[1])
        return (B, NB[lvl], H >> lvl, W >> lvl)
    lvl = int(re.search(r"\d", name).group()) - 1
    return (B, SB[lvl], H >> lvl, W >> lvl)


def run_with_plan(torch, model, fn):
    model.profile(True)
    out = fn()
    torch.cuda.synchronize()
    plan = model.profile_plan()
    assert [p[0] for p in plan] == [r[0] for r in model.profile_read()]      # the same records, in the same order
    model.profile(False)
    return out, plan


def collect(torch, model, arch, precision, x):
    """Everything one engine computes for x: the fused forward's four outputs, then (intermediates kept) the logits and every
    stored plane of every node, and the plan report of both forwards."""
    B, _, H, W = x.shape
    (mask, cable, tape, logits), plan_fused = run_with_plan(torch, model, lambda: model.segment(x, return_logits=True, return_class_masks=True))
    got = {"logits": logits.clone(), "mask": mask.clone(), "cable": cable.clone(), "tape": tape.clone()}
    model.debug_keep_intermediates(True)
    kept, plan_kept = run_with_plan(torch, model, lambda: model(x))
    got["logits (intermediates kept)"] = kept.clone()
    for name in (NODES if arch == "nested" else SIMPLE_NODES):
        for pl in planes_of(precision):
            got[f"node {name}{pl}"] = torch.from_numpy(read_plane(model, name + pl, node_shape(arch, name, B, H, W)))
    model.debug_keep_intermediates(False)
    assert model.status() == 0
    return got, plan_fused + plan_kept


def differences(n, base, got):
    """One line per tensor that is not bitwise the baseline's, in network order: the first is the layer to look at."""
    import torch
    out = []
    for key in [k for k in base if k.startswith("node ")] + [k for k in base if not k.startswith("node ")]:
        a, b = base[key], got[key]
        if not torch.equal(a, b):
            idx = np.argwhere((a != b).cpu().numpy()).tolist()
            out.append(f"n={n} {key}: {len(idx)} of {a.numel()} elements differ, first at {tuple(idx[0])}, last at {tuple(idx[-1])}")
    return out


def family(label):
    """The kernel family of a profile label (unetpp_abi.hip writes the kernel's template arguments into it)."""
    kern = label.split("|")[1]
    if kern.startswith("conv3x3_ws_uprows_kernel"):
        return "low-row"
    if kern.startswith("tapmm_ws_kernel"):
        return "gemm"
    if kern.startswith("conv3x3_bias_relu_kernel"):
        return "lock-step"
    if kern.startswith("conv3x3_ws_kernel<"):
        _, pool, head, upf, c0f, nw, _, _, cat2 = [a.strip() for a in kern[kern.index("<") + 1:kern.rindex(">")].split(",")]
        if c0f == "true":
            return "first block"
        if head == "true":
            return "head"
        if upf == "true":
            return "up 1x4" if nw == "1" else "up 2x2"
        if cat2 == "true":
            return "two-source"
        return "pool" if pool == "true" else "plain"
    return None


def layer_geometry(arch, label, B, H, W):
    """(level, H, W, Cout) of the conv a label names ('conv2_2.conv1...', 'enc3.0', 'dec1.2')."""
    name = label.split("|")[0]
    if arch == "nested":
        lvl = int(re.search(r"conv(\d)_\d", name).group(1))
        return lvl, H >> lvl, W >> lvl, NB[lvl]
    lvl = int(re.search(r"(?:enc|dec)(\d)", name).group(1)) - 1
    return lvl, H >> lvl, W >> lvl, SB[lvl]


_inputs, _sweeps = {}, {}


def inputs(key, syn, oracle):
    """x, weights and the oracle's logits of a configuration; shapes and weights are shared, so computed once per shape."""
    arch, C, B, H, W, _, _ = CONFIGS[key]
    k = (arch, C, B, H, W)
    if k not in _inputs:
        x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 11 + H))
        if arch == "nested":
            sd = syn.make_state_dict(C, 3, False, 2)
            ref = oracle.torch_forward(sd, x)
        else:
            sd = syn.make_simple_state_dict(C, 3, 2)
            ref = oracle.simple_unet_torch_forward(sd, x)
        _inputs[k] = (x, sd, ref)
    return _inputs[k]


def sweep(key, torch, syn, oracle):
    """One configuration: the baseline engine (device's own CU count) and one engine per n of N_PLANS, all with UNETPP_KSPLIT=1.
    Returns what the tests assert on; computed once per configuration."""
    if key in _sweeps:
        return _sweeps[key]
    arch, C, B, H, W, precision, extra = CONFIGS[key]
    x, sd, ref = inputs(key, syn, oracle)
    xt = torch.from_numpy(x).cuda()
    base_model = make_engine(torch, arch, C, sd, B, (H, W), precision, xt, dict(extra, UNETPP_KSPLIT="1"))
    base, base_plan = collect(torch, base_model, arch, precision, xt)
    del base_model
    res = {"base": base, "base_plan": base_plan, "plans": {}, "diffs": [], "ref": ref, "x": x, "sd": sd}
    for n in N_PLANS:
        m = make_engine(torch, arch, C, sd, B, (H, W), precision, xt, dict(extra, UNETPP_KSPLIT="1", UNETPP_PLAN_CUS=n))
        got, plan = collect(torch, m, arch, precision, xt)
        del m
        res["plans"][n] = plan
        res["diffs"] += differences(n, base, got)
    _sweeps[key] = res
    return res


def check_baseline_against_oracle(key, res, oracle):
    arch, C, B, H, W, precision, _ = CONFIGS[key]
    ref = res["ref"]
    ref_mask = oracle.masks_from_logits(ref)[0]
    lg, mk = res["base"]["logits"].cpu().numpy(), res["base"]["mask"].cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    if precision == "exact":
        err, flips, unexplained = report(lg, mk, ref, ref_mask, oracle)
        print(f"{key}: baseline max|dlogit|={err:.3e} flips={flips}")
        # test_random_shapes_against_oracle / test_simple_unet_random_shapes_against_oracle
        assert err < (2e-5 if arch == "nested" else 5e-5) * scale and unexplained == 0, (key, err, flips)
    elif precision == "exact8":
        if arch == "nested":
            gate(key, lg, mk, ref, ref_mask, oracle)
        else:                   # test_exact8_simple_unet_random_shapes_and_batch_rows
            gate(key, lg / scale, mk, ref / scale, ref_mask, oracle)
    else:                       # tests/test_gpu_fast.py, test_end_to_end_against_the_emulation
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import fast_emulation as fe
        emu, nd = fe.fast_forward(res["sd"], res["x"], return_nodes=True)
        _, S = fe.head_generic(fe._t(nd["x0_4"]), *fe._head_wb(res["sd"]))
        err, emu_err = float(np.abs(lg - ref).max()), float(np.abs(emu - ref).max())
        print(f"{key}: baseline max|device - oracle|={err:.3e}, max|emulation - oracle|={emu_err:.3e}")
        assert err <= 2 * emu_err + 4 * fe.GAMMA["head"] * float(S.max())


def check_plans(key, res, torch):
    """(b), per configuration: what the plan report must say about every launch."""
    arch, C, B, H, W, precision, _ = CONFIGS[key]
    cus = device_cus(torch)
    persistent = lambda plan: [p for p in plan if p[1] > 0]
    for name, grid, tiles, ks, rows in persistent(res["base_plan"]):
        assert family(name) is not None, name
        assert tiles <= cus and grid == tiles and ks == 1, f"baseline {name}: grid {grid}, tiles {tiles}: a workgroup would walk"
    assert [p[0] for p in res["base_plan"] if p[1] == 0 and family(p[0])] == []     # every persistent kernel reports its plan
    for n, plan in res["plans"].items():
        if n <= 5:      # every persistent launch walks -- but for the launches named in ONE_TILE_PER_IMAGE, exactly those
            still = {name.split("|")[0] for name, grid, tiles, ks, rows in persistent(plan) if tiles <= grid}
            assert still == ONE_TILE_PER_IMAGE.get((key, n), set()), f"n={n}: nothing walks in {sorted(still)}"
        for name, grid, tiles, ks, rows in persistent(plan):
            fam = family(name)
            assert fam is not None and ks == 1, (n, name, ks)
            assert 1 <= grid <= (2 * n if fam == "lock-step" else n), (n, name, grid)
            assert grid in ((min(tiles, n), min(tiles, 2 * n)) if fam == "lock-step" else (min(tiles, n),)), (n, name, grid, tiles)
            # the 8-row tiles of the lock-step kernel (small_grid_rows): pool-free, head-free, not Cout = 32, fewer 16-row tiles than CUs
            if fam == "lock-step":
                targs = [a.strip() for a in name[name.index("<") + 1:name.rindex(">")].split(",")]
                nw, pool, head, upf = int(targs[2]), targs[5] == "true", targs[6] == "true", targs[7] == "true"
                assert int(targs[3]) == rows
                _, h, w, cout = layer_geometry(arch, name, B, H, W)
                tiles16 = B * ((w + 31) // 32) * ((h + 15) // 16) * (cout // (32 * nw))
                want = 1 if not (pool or head or upf or nw == 1) and tiles16 < n else 2
                assert rows == want, (n, name, rows, want, tiles16)
                assert tiles == B * ((w + 31) // 32) * ((h + 8 * rows - 1) // (8 * rows)) * (cout // (32 * nw)), (n, name, tiles)
        # the up-sum's 4-row tiles: when the 16-row tiles would not fill the planned CUs (unetpp_abi.hip, OP_UPSUM)
        for name, *_ in plan:
            if ".up-sum|" in name:
                _, h, w, cout = layer_geometry(arch, name, B, H, W)
                blocks16 = ((w + 31) // 32) * ((h + 15) // 16) * (cout // 32) * B
                assert name.endswith(f"upsum_kernel<1, {4 if blocks16 <= n else 16}>"), (n, name, blocks16)


@pytest.mark.parametrize("key", list(CONFIGS))
def test_the_walk_changes_no_bit(key, torch_cuda, syn, oracle):
    """(a) and the per-launch half of (b) for one configuration."""
    res = sweep(key, torch_cuda, syn, oracle)
    check_baseline_against_oracle(key, res, oracle)
    check_plans(key, res, torch_cuda)
    assert res["diffs"] == [], "\n".join(res["diffs"])


def test_every_kernel_family_walks_ragged_and_permuted(torch_cuda, syn, oracle):
    """(b) over the whole sweep: every family has a launch whose last round is ragged (tiles % grid != 0, more tiles than
    workgroups) and one that takes the XCD slot permutation (grid % 8 == 0) over two or more rounds."""
    ragged, permuted = {f: [] for f in FAMILIES}, {f: [] for f in FAMILIES}
    switched = {"upsum 4": 0, "upsum 16": 0, "lock-step rows 1": 0, "lock-step rows 2": 0}
    for key in CONFIGS:
        res = sweep(key, torch_cuda, syn, oracle)
        for n, plan in res["plans"].items():
            for name, grid, tiles, ks, rows in plan:
                if ".up-sum|" in name:
                    switched["upsum 4" if name.endswith(", 4>") else "upsum 16"] += 1
                fam = family(name)
                if grid == 0 or fam is None:
                    continue
                if fam == "lock-step":
                    switched[f"lock-step rows {rows}"] += 1
                if tiles > grid and tiles % grid:
                    ragged[fam].append((key, n, name, grid, tiles))
                if grid % 8 == 0 and tiles > grid:
                    permuted[fam].append((key, n, name, grid, tiles))
    for fam in FAMILIES:
        print(f"{fam}: {len(ragged[fam])} ragged walks, {len(permuted[fam])} permuted walks of two or more rounds")
    assert [f for f in FAMILIES if not ragged[f]] == [], "families without a ragged walk"
    assert [f for f in FAMILIES if not permuted[f]] == [], "families without a permuted walk of two or more rounds"
    assert all(switched.values()), switched          # both sides of the up-sum's and of the lock-step kernel's tile-height switch ran


# ---- (c) split-K under other plans --------------------------------------------------------------------------------------------

def test_split_k_under_other_plans(torch_cuda, syn, oracle):
    """2 x 96 x 160 with the default UNETPP_KSPLIT, planned for 64 and 128 CUs and for the device: by launch_ws_k's rule the
    deep levels split differently under each.  From the report: 2-, 4- and 8-way splits all occur, a pooling layer among them.
    Each plan reproduces itself bit for bit, meets the oracle bar and differs from the unsplit plan in rounding only (DESIGN.md
    5.5, the bound of test_split_k_plan_changes_rounding_only).  exact8 has no plan-to-plan bound: reproducibility and its gate
    only, the difference is printed."""
    torch = torch_cuda
    C, B, H, W = 3, 2, 96, 160
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 41))
    sd = syn.make_state_dict(C, 3, False, 2)
    ref = oracle.torch_forward(sd, x)
    ref_mask = oracle.masks_from_logits(ref)[0]
    xt = torch.from_numpy(x).cuda()
    cus = device_cus(torch)
    for precision in ("exact", "exact8"):
        unsplit = make_engine(torch, "nested", C, sd, B, (H, W), precision, xt, {"UNETPP_KSPLIT": "1"})
        _, l0 = unsplit.segment(xt, return_logits=True)
        seen, pooled_split = set(), []
        for n in (64, 128, cus):
            m = make_engine(torch, "nested", C, sd, B, (H, W), precision, xt, {"UNETPP_PLAN_CUS": n})
            (m1, l1), plan = run_with_plan(torch, m, lambda: m.segment(xt, return_logits=True))
            m2, l2 = m.segment(xt, return_logits=True)
            torch.cuda.synchronize()
            split = [(name, grid, tiles, ks) for name, grid, tiles, ks, _ in plan if ks > 1]
            print(f"{precision} n={n}: " + ", ".join(f"{name.split('|')[0]} x{ks}" for name, _, _, ks in split))
            for name, grid, tiles, ks in split:
                assert tiles <= n and grid == tiles, (n, name, grid, tiles)          # the partials hold one record per workgroup
                seen.add(ks)
                if family(name) == "pool":
                    pooled_split.append(name)
            assert torch.equal(l1, l2) and torch.equal(m1, m2), (precision, n)
            d = float((l1 - l0).abs().max())
            lg, mk = l1.cpu().numpy(), m1.cpu().numpy()
            if precision == "exact":
                err, flips, unexplained = report(lg, mk, ref, ref_mask, oracle)
                print(f"  max|dlogit| against the oracle {err:.3e}, flips {flips}; against the unsplit plan {d:.3e}")
                assert err < 2e-5 and unexplained == 0, (n, err)
                assert 0 < d < 5e-6, (n, d)
            else:
                gate(f"exact8 n={n}", lg, mk, ref, ref_mask, oracle)
                print(f"  exact8 n={n}: max|dlogit| against the unsplit plan {d:.3e} (no bound exists for it)")
            assert m.status() == 0
            del m
        assert {2, 4, 8} <= seen, (precision, sorted(seen))
        assert pooled_split, precision
        del unsplit


# ---- (d) split-K on concurrent internal streams -------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["exact", "exact8"])
def test_split_k_on_concurrent_streams(precision, torch_cuda, syn):
    """5 x 64 x 64 as five batch-1 passes on three internal streams with the default split-K plan: every pass splits its deep
    levels, and each slot must have partial sums and arrival counters of its own -- row i equals a single-stream engine's result
    for frame i bit for bit, twice."""
    torch = torch_cuda
    C, B, H, W = 3, 5, 64, 64
    x = torch.from_numpy(syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 21))).cuda()
    sd = syn.make_state_dict(C, 3, False, 2)
    single = make_engine(torch, "nested", C, sd, 1, (H, W), precision, x[:1], {})
    multi = make_engine(torch, "nested", C, sd, B, (H, W), precision, x, {}, micro_batch=1, streams=3)
    _, plan = run_with_plan(torch, single, lambda: single(x[:1]))
    assert any(ks > 1 for *_, ks, _ in plan), "the batch-1 plan at 64 x 64 no longer splits: this test has lost its subject"
    a, a2 = multi(x), multi(x)
    torch.cuda.synchronize()
    assert torch.equal(a, a2)
    for i in range(B):
        assert torch.equal(a[i:i + 1], single(x[i:i + 1])), i
    assert multi.status() == 0 and single.status() == 0


def test_plan_cus_above_the_device_is_refused(torch_cuda, syn):
    """No grid larger than the device's own plan is ever launched: a count above the device's is UNETPP_E_INVALID, after the
    query; the device's own count is accepted and is the default plan."""
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    cus = device_cus(torch)
    x = torch.from_numpy(syn.frames_to_chw_f32(syn.make_frames_u8(1, 32, 32, "smooth", 3))).cuda()
    sd = syn.make_state_dict(3, 3, False, 2)
    m = NestedUNet(3, deep_supervision=False, max_batch=1, max_hw=(32, 32)).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    with plan_env(UNETPP_PLAN_CUS=cus + 1):
        with pytest.raises(RuntimeError, match=rf"unetpp_create failed \(-1\): UNETPP_PLAN_CUS={cus + 1} exceeds the device's {cus} compute units"):
            m.eval()(x)
    own = make_engine(torch, "nested", 3, sd, 1, (32, 32), "exact", x, {"UNETPP_PLAN_CUS": cus})
    default = make_engine(torch, "nested", 3, sd, 1, (32, 32), "exact", x, {})
    (a, plan_own), (b, plan_default) = run_with_plan(torch, own, lambda: own(x)), run_with_plan(torch, default, lambda: default(x))
    assert plan_own == plan_default and torch.equal(a, b)
