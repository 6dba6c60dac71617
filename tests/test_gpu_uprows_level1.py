"""conv3x3_ws_uprows_kernel for Cout = 64 (csrc/conv3x3_ws.h, UR): conv1_3.conv1 of `exact` as two 32-channel tiles per 16-row
pixel tile, its 128 up channels multiplied on low-resolution rows.  Against the CPU oracle, against the 2 x 2 fused-upsample
kernel of an engine created with UNETPP_UPROWS=0, layer-wise on the device's own inputs, and for batch-row invariance.
Run on the GPU box: python -m pytest tests -m gpu"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import make_model, report, torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

UPROWS_L1 = "conv1_3.conv1+up|conv3x3_ws_uprows_kernel"
UPROWS_L0 = "conv0_4.conv1+up|conv3x3_ws_uprows_kernel"
PLAIN_L1 = "conv1_3.conv1+up|conv3x3_ws_kernel<2, false, false, true, false, 2, 2, false, false>"
PLAIN_L0 = "conv0_4.conv1+up|conv3x3_ws_kernel<2, false, false, true, false, 1, 4, false, false>"

# level 1 is H/2 x W/2 in 16 x 32 tiles.  32 x 64: one level-1 tile, all four borders; 96 x 160: a middle row tile and a half column
# tile; 160 x 96: the transposed case; 48 x 80: level-1 height 24, a row tile half outside; 64 x 192: three frames, three column tiles
CASES = [(3, 1, 32, 64), (3, 2, 96, 160), (3, 1, 160, 96), (7, 1, 48, 80), (3, 3, 64, 192)]


def _read(model, name, shape):
    from unet_amd import _lib
    out = np.empty(shape, dtype=np.float32)
    n = _lib.load().unetpp_debug_read(model._handle, name.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
    assert n == out.size, (name, n, out.size)
    return out


def _names(torch, model, xt):
    """one profiled forward: (labels, logits)"""
    model.profile(True)
    out = model(xt)
    torch.cuda.synchronize()
    names = [r[0] for r in model.profile_read()]
    model.profile(False)
    return names, out


def _layer_error(torch, model, xt, sd, B, H, W):
    """conv1_3.conv1 as the engine stored it (x1_3a) against the float64 layer on the engine's own stored inputs x1_0 and x2_2,
    relative to the layer's largest value; debug_keep_intermediates moves conv0_4.conv1 to the plain kernel and nothing else"""
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import exact8_emulation as em
    model.debug_keep_intermediates(True)
    names, _ = _names(torch, model, xt)
    sk, lo = _read(model, "x1_0", (B, 64, H // 2, W // 2)), _read(model, "x2_2", (B, 128, H // 4, W // 4))
    got = _read(model, "x1_3a", (B, 64, H // 2, W // 2))
    model.debug_keep_intermediates(False)
    T = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    w, b = em._fold(sd, "conv1_3.conv1")
    up = F.interpolate(T(lo), scale_factor=2, mode="bilinear", align_corners=True)
    ref = torch.relu(F.conv2d(torch.cat([T(sk), up], 1), w.to(torch.float64), padding=1) + b.to(torch.float64)[None, :, None, None]).numpy()
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max()), names


@pytest.mark.parametrize("C,B,H,W", CASES, ids=lambda v: str(v))
def test_uprows_level1_against_oracle_2x2_kernel_layer_and_row_order(C, B, H, W, torch_cuda, syn, oracle, monkeypatch):
    """The layer-wise bar: there is no `exact` sibling of test_gpu_exact8's per-layer check, so the 2 x 2 kernel's own error on the
    same stored inputs (the UNETPP_UPROWS=0 engine) is measured in the test and the low-row kernel may have twice that.
    Measured (low-row kernel, 2 x 2 kernel), max |x1_3a - float64 layer| of the layer's largest value:
      (3,1,32,64)  (8.8e-07, 1.74e-06)    (3,2,96,160) (1.05e-06, 1.69e-06)    (3,1,160,96) (1.28e-06, 1.33e-06)
      (7,1,48,80)  (1.17e-06, 1.35e-06)   (3,3,64,192) (1.03e-06, 1.56e-06)
    and the logits of the two plans differ by 2.4e-06 ... 3.8e-06."""
    torch = torch_cuda
    frames = syn.make_frames_u8(B, H, W, "smooth", 100 * H + W)
    x = syn.frames_to_chw_f32(frames)
    model, sd = make_model(C, C == 3, 11, "exact", syn, B, (H, W))
    ref = oracle.torch_forward(sd, x)
    xt = torch.from_numpy(x).cuda()

    model(xt)                                              # creates the engine
    model.profile(True)
    mask, logits = model.segment(xt, return_logits=True)
    torch.cuda.synchronize()
    names = [r[0] for r in model.profile_read()]
    model.profile(False)
    assert UPROWS_L1 in names and UPROWS_L0 in names, names

    # the random-shape sweep's bar (test_gpu_parity.test_random_shapes_against_oracle)
    err, flips, unexplained = report(logits.cpu().numpy(), mask.cpu().numpy(), ref, oracle.masks_from_logits(ref)[0], oracle)
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"uprows level 1 {C}c {B}x{H}x{W}: max|dlogit|={err:.3e} scale={scale:.3f} flips={flips} unexplained={unexplained}")
    assert err < 2e-5 * scale and unexplained == 0, (err, scale, flips)

    # the 2 x 2 kernel for this layer: an engine created with UNETPP_UPROWS=0 (level 0 only)
    monkeypatch.setenv("UNETPP_UPROWS", "0")
    other, _ = make_model(C, C == 3, 11, "exact", syn, B, (H, W))
    other(xt)                                              # creates the engine: the plan is fixed here
    monkeypatch.delenv("UNETPP_UPROWS")
    names0, logits0 = _names(torch, other, xt)
    assert PLAIN_L1 in names0 and UPROWS_L0 in names0 and UPROWS_L1 not in names0, names0
    d = float((logits0 - logits).abs().max())
    print(f"uprows level 1 vs 2 x 2 fused-upsample kernel: max|dlogit|={d:.3e}")
    assert d < 2e-5, d                                     # two plans of one layer (test_alternative_kernel_paths_agree)

    # the layer itself, on the device's own inputs; level 1 keeps its plan under debug_keep_intermediates, level 0 does not
    e_ur, names_k = _layer_error(torch, model, xt, sd, B, H, W)
    e_22, names_k0 = _layer_error(torch, other, xt, sd, B, H, W)
    assert UPROWS_L1 in names_k and PLAIN_L0 in names_k and UPROWS_L0 not in names_k, names_k
    assert PLAIN_L1 in names_k0 and PLAIN_L0 in names_k0, names_k0
    print(f"conv1_3.conv1 + upsample, max|x1_3a - float64 layer| of the largest value: low rows {e_ur:.3e}, 2 x 2 kernel {e_22:.3e}")
    assert e_ur <= 2 * e_22, (e_ur, e_22)

    # a frame's result does not depend on its row of the batch: the permuted batch, row for row, bit for bit
    perm = torch.arange(B - 1, -1, -1, device=xt.device)
    again = model(xt[perm].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(again, logits[perm])
    assert model.status() == 0 and other.status() == 0


@pytest.mark.parametrize("env", [{"UNETPP_UPROWS": "0"}, {"UNETPP_UPROWS": "none"}])
def test_uprows_plans_agree(env, torch_cuda, syn, oracle, monkeypatch):
    """UNETPP_UPROWS, read when an engine is created, picks which decoder levels multiply their up channels on low-resolution rows
    (absent: 0 and 1; "0": level 0 only; "none": neither).  Each plan passes the default path's parity bar and agrees with it to
    rounding (test_gpu_parity.test_alternative_kernel_paths_agree, same frames and weights)."""
    torch = torch_cuda
    frames = syn.make_frames_u8(2, 96, 160, "smooth", 41)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    base, sd = make_model(3, True, 2, "exact", syn, 2, (96, 160))
    ref = oracle.torch_forward(sd, syn.frames_to_chw_f32(frames))
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    m0, l0 = base.segment(x, return_logits=True)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    alt, _ = make_model(3, True, 2, "exact", syn, 2, (96, 160))
    m1, l1 = alt.segment(x, return_logits=True)
    names, _ = _names(torch, alt, x)
    torch.cuda.synchronize()
    assert PLAIN_L1 in names and (UPROWS_L0 if env["UNETPP_UPROWS"] == "0" else PLAIN_L0) in names, names
    for name, lg, mk in (("default", l0, m0), (str(env), l1, m1)):
        err, flips, unexplained = report(lg.cpu().numpy(), mk.cpu().numpy(), ref, ref_mask, oracle)
        print(f"{name}: max|dlogit|={err:.3e} flips={flips}")
        assert err < 2e-5 and unexplained == 0
    assert float((l0 - l1).abs().max()) < 2e-5
    assert alt.status() == 0 and base.status() == 0
