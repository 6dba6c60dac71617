"""Every launch the engine makes, pinned: label, work figures and plan of each profile record against a recording of the
commit named in tests/golden/README_launch_records.txt (scripts/make_golden_launch_records.py writes it).

The host code of unetpp_abi.hip decides, per launch, the kernel instantiation, its label, the flops and bytes it reports and the
persistent plan (grid, tiles, split-K share count, rows per wave).  A refactoring of that code must reproduce all of it; this
file says so for every configuration of the plan sweep, for batch 1 (where split-K fires), uint8 input, two passes on two
internal streams and the deep-supervision outputs.  Engines are planned for 8 and for 64 compute units (UNETPP_PLAN_CUS), so the
records are the same on any device with at least 64.

Labels and plans must be equal; flops and bytes agree within 1e-12 relative (they are sums of doubles: their order is not
behaviour).
Run on the GPU box:  python -m pytest tests -m gpu"""
import json
import os

import pytest

from conftest import GOLDEN
from test_gpu_plan_sweep import CONFIGS, device_cus, plan_env

pytestmark = pytest.mark.gpu

PLAN_CUS = (8, 64)
FIXTURE = os.path.join(GOLDEN, "launch_records.json")
_S1 = dict(arch="nested", C=7, H=48, W=80)

# name -> arch, classes, batch, H, W, precision; switches: further plan switches; engine: further constructor arguments;
# u8: uint8 NHWC frames as input; ds: a deep-supervision engine, asked for outputs 0-3 and for the pruned output 2
CASES = {k: dict(arch=a, C=C, B=B, H=H, W=W, precision=p, switches=sw) for k, (a, C, B, H, W, p, sw) in CONFIGS.items()}
CASES.update({
    "S1-b1-exact": dict(_S1, B=1, precision="exact"),
    "S1-b1-exact8": dict(_S1, B=1, precision="exact8"),
    "S1-b1-exact-u8": dict(_S1, B=1, precision="exact", u8=True),
    "S1-b3-exact-two-passes": dict(_S1, B=3, precision="exact", engine=dict(micro_batch=2, streams=2)),
    "S1-ds-exact": dict(_S1, B=3, precision="exact", ds=True),
    "S1-ds-fast": dict(_S1, B=3, precision="fast", ds=True),
})


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


def records_of(torch, model, fn):
    """[[label, flops, bytes, grid, tiles, ksplit, rows]] of the launches fn() makes."""
    model.profile(True)
    fn()
    torch.cuda.synchronize()
    work, plan = model.profile_read(), model.profile_plan()
    model.profile(False)
    assert [p[0] for p in plan] == [r[0] for r in work]
    return [[name, flops, nbytes, *p[1:]] for (name, _, flops, nbytes), p in zip(work, plan)]


def record_case(torch, syn, key, cus):
    """{pass name: records} of one configuration on an engine planned for `cus` compute units: the fused forward first, then
    the forward with intermediates kept."""
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    c = CASES[key]
    B, H, W, C, ds = c["B"], c["H"], c["W"], c["C"], c.get("ds", False)
    frames = syn.make_frames_u8(B, H, W, "smooth", 11 + H)
    x = torch.from_numpy(frames if c.get("u8") else syn.frames_to_chw_f32(frames)).cuda()
    kw = dict(precision=c["precision"], max_batch=B, max_hw=(H, W), **c.get("engine", {}))
    if c["arch"] == "nested":
        m = NestedUNet(C, deep_supervision=ds, **kw).to("cuda:0")
        m.load_state_dict(syn.make_state_dict(C, 3, ds, 2), strict=True)
    else:
        m = SimpleUNet(num_classes=C, num_channels=3, **kw).to("cuda:0")
        m.load_state_dict(syn.make_simple_state_dict(C, 3, 2), strict=True)
    m.eval()
    with plan_env(**dict(c.get("switches", {}), UNETPP_PLAN_CUS=cus)):
        m(x)                      # the first forward creates the engine
    out = {}
    if ds:
        out["outputs 0-3"] = records_of(torch, m, lambda: m.forward_deep_supervision(x))
        out["pruned output 2"] = records_of(torch, m, lambda: m.segment(x, output=2))
    else:
        out["fused"] = records_of(torch, m, lambda: m.segment(x, return_logits=True, return_class_masks=True))
    m.debug_keep_intermediates(True)
    out["intermediates kept"] = records_of(torch, m, (lambda: m.forward_deep_supervision(x)) if ds else (lambda: m(x)))
    assert m.status() == 0
    return out


def differences(where, want, got):
    if len(want) != len(got):
        return [f"{where}: {len(got)} launches, recorded {len(want)}: {[r[0] for r in got]} against {[r[0] for r in want]}"]
    out = []
    for i, (a, b) in enumerate(zip(want, got)):
        if a[0] != b[0]:
            out.append(f"{where} launch {i}: label {b[0]!r}, recorded {a[0]!r}")
        if list(a[3:]) != list(b[3:]):
            out.append(f"{where} launch {i} {a[0]}: plan (grid, tiles, ksplit, rows) {b[3:]}, recorded {a[3:]}")
        for what, u, v in (("flops", a[1], b[1]), ("bytes", a[2], b[2])):
            if abs(u - v) > 1e-12 * max(abs(u), abs(v)):
                out.append(f"{where} launch {i} {a[0]}: {what} {v!r}, recorded {u!r}")
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)["records"]


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(f"{key} cus={n}" for key in CASES for n in PLAN_CUS)


@pytest.mark.parametrize("key", list(CASES))
def test_launch_records(key, torch_cuda, syn, golden):
    assert device_cus(torch_cuda) >= max(PLAN_CUS)
    diffs = []
    for n in PLAN_CUS:
        want, got = golden[f"{key} cus={n}"], record_case(torch_cuda, syn, key, n)
        assert sorted(want) == sorted(got)
        for name in want:
            diffs += differences(f"{key} cus={n}, {name}", want[name], got[name])
    assert diffs == [], "\n".join(diffs)
