"""precision='exact8' (include/unetpp.h UNETPP_PREC_EXACT8): the parity-gated mode that issues two thirds of EXACT's
matrix-pipe cycles — hi*hi in fp16, the two small cross terms of the split product from 8-bit operands in one block-scaled
K = 64 MFMA per tap pair (csrc/conv3x3_ws.h).  Replaces the arithmetic of ConvBlock (reference src/models/unetpp.py:17-26).

Bar (north_star): logits within 1e-3 of the fp32 reference, and every mask pixel that differs from the reference's must be
a near-tie of the reference's own logits (top-2 margin below twice the logit error).  Unlike 'exact' (1e-5-class) this mode
does flip near-tie pixels; every test prints how many and how close they were.
Run on the GPU box:  python -m pytest tests -m gpu"""
import hashlib

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3     # north_star: logits within 1e-3 (fp32)
NODES = ("x0_0", "x1_0", "x2_0", "x3_0", "x4_0", "x3_1", "x2_2", "x1_3", "x0_4")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


def make_model(C, ds, sd, B, hw, precision="exact8"):
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(C, deep_supervision=ds, precision=precision, max_batch=B, max_hw=hw).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    return m.eval()


def gate(tag, logits, mask, ref_logits, ref_mask, oracle, tol=LOGIT_TOL):
    """the north_star bar for one result; returns (err, flips)"""
    err = float(np.abs(logits - ref_logits).max())
    margin = oracle.top2_margin(ref_logits)
    flips = mask != ref_mask
    worst = float(margin[flips].max()) if flips.any() else 0.0
    print(f"{tag}: max|dlogit|={err:.3e}  flips={int(flips.sum())}/{flips.size}  largest reference margin at a flip={worst:.2e}")
    assert err < tol, f"{tag}: logit error {err:.3e} above {tol}"
    assert not (flips & (margin > 2 * err + 1e-7)).any(), f"{tag}: a flipped pixel is not a near-tie"
    return err, int(flips.sum())


@pytest.mark.parametrize("tag", ["s_c3_32x32", "s_c3_64x64", "s_c7_48x80", "s_c3_128x96"])
def test_exact8_matches_golden_small(tag, torch_cuda, syn, oracle):
    torch = torch_cuda
    g = load_golden(tag)
    B, H, W, C = int(g["B"]), int(g["H"]), int(g["W"]), int(g["num_classes"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha"])
    sd = syn.make_state_dict(C, 3, bool(g["deep_supervision"]), int(g["wseed"]))
    model = make_model(C, bool(g["deep_supervision"]), sd, B, (H, W))
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    mask, cable, tape, logits = model.segment(x, return_logits=True, return_class_masks=True)
    m_u8, l_u8 = model.segment(torch.from_numpy(frames).cuda(), return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(l_u8, logits) and torch.equal(m_u8, mask)          # the uint8 BGR entry computes the same bits
    gate(tag, logits.cpu().numpy(), mask.cpu().numpy(), g["logits"], g["mask"], oracle)
    mk = mask.cpu().numpy()
    assert np.array_equal(cable.cpu().numpy(), (mk == 1).astype(np.uint8)) and np.array_equal(tape.cpu().numpy(), (mk == 2).astype(np.uint8))
    if tag == "s_c3_32x32":                 # layer by layer against the reference's intermediates: where an error enters
        model.debug_keep_intermediates(True)
        logits_unfused = model(x)
        torch.cuda.synchronize()
        # the unfused head reads x0_4 back from its stored (hi, lo8) form: 2^-14 relative instead of the fused head's fp32 registers
        assert float((logits_unfused - logits).abs().max()) < 3e-4
        for name in NODES:
            got = model.debug_activation(name, B, H, W)
            ref = g["t_" + name]
            rel = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"  {name}: max error {rel:.1e} of the node's largest value")
            assert rel < 3e-4, name        # measured 2e-5 ... 7e-5 (exact: 1e-6, fast: 1e-3)
    assert model.status() == 0


def _b16_inputs(syn, g):
    kinds = [str(k) for k in g["kinds"]]
    frames = np.stack([syn.make_frame_u8(512, 512, i, kinds[i % len(kinds)], int(g["fseed"])) for i in range(int(g["B"]))])
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha"])
    return frames


def test_exact8_config2_batch16_against_reference_fixture(torch_cuda, syn, oracle):
    """BASELINE config 2 at its stated batch of 16 against the reference-generated fixture: 8x-subsampled logits of all 16
    frames within 1e-3, every differing mask pixel on the fixture's near-tie list (reference margin < 1e-3), per-layer
    samples of frames 0-1, and the full-resolution gate against the oracle for frames 0-1."""
    torch = torch_cuda
    g = load_golden("b_c3_512x512_b16")
    frames = _b16_inputs(syn, g)
    sd = syn.make_state_dict(3, 3, True, int(g["wseed"]))
    model = make_model(3, True, sd, 16, (512, 512))
    x = syn.frames_to_chw_f32(frames)
    xt = torch.from_numpy(x).cuda()
    mask, logits = model.segment(xt, return_logits=True)
    torch.cuda.synchronize()
    lg = logits.cpu().numpy(); mk = mask.cpu().numpy()
    sub = float(np.abs(lg[:, :, ::8, ::8] - g["logits_sub8"]).max())
    diff = np.argwhere(mk != g["mask"])
    ties = {tuple(t) for t in g["tie_idx"].tolist()}
    print(f"config 2, B=16, exact8: sub8 max|dlogit|={sub:.3e}, {len(diff)} of {mk.size} mask pixels differ "
          f"({len(diff) / mk.size:.2e} per pixel), near-ties listed in the fixture: {len(ties)}")
    assert sub < LOGIT_TOL
    assert all(tuple(d) in ties for d in diff.tolist())          # only listed near-tie pixels (reference margin < 1e-3) may differ
    ref = oracle.torch_forward(sd, x[:2])
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    gate("config 2 frames 0-1 vs oracle", lg[:2], mk[:2], ref, ref_mask, oracle)
    for i in (4, 12):                                            # batch-row invariance, bitwise (4 frames: no split-K plan either)
        mi, li = model.segment(xt[i:i + 4], return_logits=True)
        assert torch.equal(li, logits[i:i + 4]) and torch.equal(mi, mask[i:i + 4])
    # one frame alone takes the split-K plan at levels 3-4 (other summation order, then other roundings of the stored planes)
    m1, l1 = model.segment(xt[1:2], return_logits=True)
    torch.cuda.synchronize()
    print(f"  frame 1 alone (split-K plan) vs its batch row: max|dlogit|={float((l1 - logits[1:2]).abs().max()):.3e}")
    gate("config 2 frame 1 alone vs oracle", l1.cpu().numpy(), m1.cpu().numpy(), ref[1:2], ref_mask[1:2], oracle)
    model.debug_keep_intermediates(True)
    model(xt[:2])
    torch.cuda.synchronize()
    for name in NODES:
        got = model.debug_activation(name, 2, 512, 512)
        ys, xs = g["p_" + name][:, 0], g["p_" + name][:, 1]
        ref_n = g["t_" + name]
        rel = float(np.abs(got[:, :, ys, xs] - ref_n).max() / np.abs(ref_n).max())
        print(f"  {name}: max error {rel:.1e} of the largest sampled value")
        assert rel < 3e-4, name
    assert model.status() == 0


def test_exact8_config5_1024_batch8(torch_cuda, syn, oracle):
    """BASELINE config 5 (3-class 1024x1024, batch 8): frame 0 against the reference's fixture, the others by batch-row
    invariance (bitwise)."""
    torch = torch_cuda
    g = load_golden("b_c3_1024x1024")
    frames = syn.make_frames_u8(8, 1024, 1024, "smooth", int(g["fseed"]))
    assert hashlib.sha256(frames[:1].tobytes()).hexdigest() == str(g["frames_sha"])
    model = make_model(3, True, syn.make_state_dict(3, 3, True, int(g["wseed"])), 8, (1024, 1024))
    xu8 = torch.from_numpy(frames).cuda()
    mask, logits = model.segment(xu8, return_logits=True)
    torch.cuda.synchronize()
    sub = float(np.abs(logits[:1, :, ::8, ::8].cpu().numpy() - g["logits_sub8"]).max())
    diff = np.argwhere(mask[:1].cpu().numpy() != g["mask"])
    ties = {tuple(t) for t in g["tie_idx"].tolist()}
    print(f"config 5, B=8, exact8: frame 0 sub8 max|dlogit|={sub:.3e}, {len(diff)} of {1024 * 1024} mask pixels differ")
    assert sub < LOGIT_TOL and all(tuple(d) in ties for d in diff.tolist())
    for i in (1, 4, 7):
        mi, li = model.segment(xu8[i:i + 1], return_logits=True)
        assert torch.equal(li, logits[i:i + 1]) and torch.equal(mi, mask[i:i + 1])
    assert model.status() == 0


def test_exact8_config4_7class_448x800_batch32(torch_cuda, syn, oracle):
    """BASELINE config 4 (7-class 448x800, batch 32): frame 0 against the reference's fixture; frames 0 and 31 of the batch
    against the oracle on the host; batch-row invariance."""
    torch = torch_cuda
    g = load_golden("b_c7_448x800")
    frames = syn.make_frames_u8(32, 448, 800, "smooth", int(g["fseed"]))
    assert hashlib.sha256(frames[:1].tobytes()).hexdigest() == str(g["frames_sha"])
    sd = syn.make_state_dict(7, 3, False, int(g["wseed"]))
    model = make_model(7, False, sd, 32, (448, 800))
    fu8 = torch.from_numpy(frames).cuda()
    mask, logits = model.segment(fu8, return_logits=True)
    torch.cuda.synchronize()
    sub = float(np.abs(logits[:1, :, ::8, ::8].cpu().numpy() - g["logits_sub8"]).max())
    diff = np.argwhere(mask[:1].cpu().numpy() != g["mask"])
    ties = {tuple(t) for t in g["tie_idx"].tolist()}
    print(f"config 4, B=32, exact8: frame 0 sub8 max|dlogit|={sub:.3e}, {len(diff)} mask pixels differ")
    assert sub < LOGIT_TOL and all(tuple(d) in ties for d in diff.tolist())
    x = syn.frames_to_chw_f32(frames[[0, 31]])
    ref = oracle.torch_forward(sd, x)
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    gate("config 4 frames 0, 31 vs oracle", logits[[0, 31]].cpu().numpy(), mask[[0, 31]].cpu().numpy(), ref, ref_mask, oracle)
    m5 = model.segment(fu8[4:6])
    assert torch.equal(mask[4:6], m5)
    assert model.status() == 0


def test_exact8_trained_like_weights_512(torch_cuda, syn, oracle):
    """Weights with the statistics only trained checkpoints show (running_var = 1e-8 on near-dead channels, negative / zero /
    large gamma) at 512x512, batch 2 — a size where the deep layers span many tiles — against the oracle on the host, for
    'exact' (2e-5-class) and 'exact8' (1e-3 gate)."""
    torch = torch_cuda
    sd = syn.make_trained_like_state_dict(3, 3, True, 2)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(2, 512, 512, "smooth", 7))
    ref = oracle.torch_forward(sd, x)
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    xt = torch.from_numpy(x).cuda()
    for prec, tol in (("exact", 2e-5 * max(1.0, float(np.abs(ref).max()))), ("exact8", LOGIT_TOL)):
        model = make_model(3, True, sd, 2, (512, 512), precision=prec)
        mask, logits = model.segment(xt, return_logits=True)
        torch.cuda.synchronize()
        gate(f"trained-like 512x512 {prec}", logits.cpu().numpy(), mask.cpu().numpy(), ref, ref_mask, oracle, tol=tol)
        assert model.status() == 0
        del model


@pytest.mark.parametrize("C,B,H,W", [(3, 1, 16, 16), (3, 3, 16, 80), (7, 2, 80, 16), (3, 2, 112, 144), (8, 1, 16, 48), (1, 1, 16, 32),
                                     (3, 1, 16, 2048), (3, 1, 2048, 16)])
def test_exact8_ragged_shapes_against_oracle(C, B, H, W, torch_cuda, syn, oracle):
    """Minimum size, single rows / columns of tiles, widths and heights that are not multiples of the tile."""
    torch = torch_cuda
    ds = C == 3
    frames = syn.make_frames_u8(B, H, W, "uniform", 100 + H + W)
    x = syn.frames_to_chw_f32(frames)
    sd = syn.make_state_dict(C, 3, ds, 2)
    model = make_model(C, ds, sd, B, (H, W))
    ref = oracle.torch_forward(sd, x)
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    mask, logits = model.segment(torch.from_numpy(frames).cuda(), return_logits=True)
    torch.cuda.synchronize()
    gate(f"C={C} {B}x{H}x{W}", logits.cpu().numpy(), mask.cpu().numpy(), ref, ref_mask, oracle)
    assert model.status() == 0


def test_exact8_probabilities_and_rules(torch_cuda, syn, oracle):
    """The fused softmax + class rules run on the exact8 logits: probabilities within 1e-3 / 4 of the reference's, rule masks
    equal wherever no probability sits within that distance of a decision boundary."""
    from test_oracle_golden import RULE_CASES
    torch = torch_cuda
    g = load_golden("s_c3_128x96")
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    model = make_model(3, True, syn.make_state_dict(3, 3, True, int(g["wseed"])), B, (H, W))
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    probs = model.predict_proba(x)
    torch.cuda.synchronize()
    ref_p = np.transpose(g["probs_hwc"], (0, 3, 1, 2))
    perr = float(np.abs(probs.cpu().numpy() - ref_p).max())
    print(f"exact8 max|dprob|={perr:.3e}")
    assert perr < 2.5e-4
    p0, p1, p2 = ref_p[:, 0], ref_p[:, 1], ref_p[:, 2]
    for key, rule, params in RULE_CASES:
        cable, tape = model.segment_thresholded(x, rule=rule, **params)
        torch.cuda.synchronize()
        diff = (cable.cpu().numpy() != g[f"rule_{key}_cable"]) | (tape.cpu().numpy() != g[f"rule_{key}_tape"])
        tc, tt, bgm = params["t_cable"], params["t_tape"], params["bg_margin"]
        ctm = params.get("ct_margin", 0.0)
        d = np.minimum.reduce([np.abs(p1 - tc), np.abs(p2 - tt), np.abs(p1 - p0 - bgm), np.abs(p2 - p0 - bgm),
                               np.abs(p0 - bgm), np.abs(p1 - p2 - ctm), np.abs(p2 - p1 - ctm), np.abs(p1 - p2),
                               np.abs(p1 - p0), np.abs(p2 - p0)])
        print(f"  {key}: differing pixels {int(diff.sum())}")
        assert not (diff & (d > 2 * perr + 1e-7)).any(), key


def test_unknown_precision_is_rejected(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    with pytest.raises(ValueError):
        NestedUNet(3, precision="exact4")


def test_exact8_tapmm_switch_agrees(torch_cuda, syn, oracle, monkeypatch):
    """UNETPP_TAPMM=none: levels 2-3 interpolate in the loader instead of taking the low-resolution GEMM — both paths inside
    the gate and close to each other."""
    torch = torch_cuda
    frames = syn.make_frames_u8(2, 96, 160, "smooth", 41)
    x = syn.frames_to_chw_f32(frames)
    sd = syn.make_state_dict(3, 3, True, 2)
    ref = oracle.torch_forward(sd, x)
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    xt = torch.from_numpy(x).cuda()
    base = make_model(3, True, sd, 2, (96, 160))
    m0, l0 = base.segment(xt, return_logits=True)
    monkeypatch.setenv("UNETPP_TAPMM", "none")
    alt = make_model(3, True, sd, 2, (96, 160))
    m1, l1 = alt.segment(xt, return_logits=True)
    torch.cuda.synchronize()
    gate("default", l0.cpu().numpy(), m0.cpu().numpy(), ref, ref_mask, oracle)
    gate("UNETPP_TAPMM=none", l1.cpu().numpy(), m1.cpu().numpy(), ref, ref_mask, oracle)
    assert float((l0 - l1).abs().max()) < LOGIT_TOL


def test_exact8_microbatch_and_streams_invariance(torch_cuda, syn, monkeypatch):
    """Micro-batching and concurrent passes on the engine's internal streams never change a bit in exact8 either (one launch
    plan: the split-K plan of small launches is switched off here; tests/test_gpu_parity.py has its own test)."""
    from unet_amd.nested_unet import NestedUNet
    torch = torch_cuda
    monkeypatch.setenv("UNETPP_KSPLIT", "1")
    frames = syn.make_frames_u8(5, 64, 96, "smooth", 21)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    sd = syn.make_state_dict(3, 3, True, 2)

    def model(**kw):
        m = NestedUNet(3, precision="exact8", max_batch=5, max_hw=(64, 96), **kw).to("cuda:0")
        m.load_state_dict(sd, strict=True)
        return m.eval()
    full, micro, multi = model(), model(micro_batch=2), model(micro_batch=1, streams=3)
    a = full(x); b = micro(x); c = full(x[3:4]); d = multi(x); d2 = multi(x)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, d) and torch.equal(a, d2) and torch.equal(a[3:4], c)
    assert full.status() == 0 and multi.status() == 0


def _read(model, name, shape):
    """unetpp_debug_read of any activation tensor of the engine (also the conv1 outputs 'x1_0a' and the pooled 'x0_0p')"""
    import ctypes
    from unet_amd import _lib
    out = np.empty(shape, dtype=np.float32)
    n = _lib.load().unetpp_debug_read(model._handle, name.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
    assert n == out.size, (name, n, out.size)
    return out


def test_exact8_layers_compute_the_documented_arithmetic(torch_cuda, syn, oracle):
    """The 1e-3 gate cannot see a wrong block scale, a swapped byte order or a dropped cross term (the terms are 2^-11 of the
    result).  oracle/exact8_emulation.py emulates DESIGN.md §3's arithmetic in float64; every KIND of layer is checked on the
    GPU's own stored inputs (read back with unetpp_debug_read): fused first block, plain conv + pool, conv after a pool,
    decoder conv with the fused upsample (level 1), decoder conv through the low-resolution GEMM (level 3), a split-K launch.
    A layer's mean deviation from the emulation must be 10x below its mean deviation from the fp32 reference's arithmetic on
    the same inputs (measured 22x with the fp32 interpolation in front, 40-90x elsewhere: what is left are e5m2 roundings of
    the residual plane that flip on fp32 summation order, 1.4-6 % of the elements); a dropped tap or a wrong scale would put
    it at that level or above."""
    import os, sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import exact8_emulation as em
    import torch.nn.functional as F
    torch = torch_cuda
    B, H, W = 2, 64, 96
    sd = syn.make_state_dict(3, 3, True, 2)
    frames = syn.make_frames_u8(B, H, W, "smooth", 7)
    x = syn.frames_to_chw_f32(frames)
    model = make_model(3, True, sd, B, (H, W))
    model.debug_keep_intermediates(True)
    model(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    rd = lambda name, c, lvl: _read(model, name, (B, c, H >> lvl, W >> lvl))
    act = lambda name, c, lvl: em.act_from_planes(rd(name + "#hi", c, lvl), rd(name + "#lo", c, lvl), rd(name + "#x8", c, lvl))
    T = lambda a: torch.from_numpy(np.asarray(a, np.float64))

    def fp32_layer(inp, name, pad=1):      # the reference's arithmetic (conv + folded BN + ReLU in float64) on the same stored inputs
        w, b = em._fold(sd, name)
        return torch.relu(F.conv2d(inp, w, padding=pad) + b[None, :, None, None])

    def check(tag, got, emu_v, ref_v):
        d_emu, d_ref, differ = em.layer_agreement(got, emu_v, ref_v)
        print(f"{tag}: mean |GPU - emulation| = {d_emu:.2e}, mean |GPU - fp32 arithmetic| = {d_ref:.2e} (of the largest value); "
              f"{differ:.2%} of the elements differ from the emulation")
        assert d_emu * 10 < d_ref, tag
        assert differ < 0.12, tag

    # fused first block: raw input -> x0_0
    v = em.first_block(x, sd)
    w1, b1 = em._fold(sd, "conv0_0.conv1")
    ref = fp32_layer(torch.relu(F.conv2d(T(x), w1, padding=1) + b1[None, :, None, None]), "conv0_0.conv2")
    check("first block", rd("x0_0", 32, 0), v, ref)
    # plain conv + fused pool: x1_0a -> x1_0, x1_0p
    a = rd("x1_0a", 64, 1)
    v = em.conv_layer(act("x1_0a", 64, 1), sd, "conv1_0.conv2")
    ref = fp32_layer(T(a), "conv1_0.conv2")
    check("conv1_0.conv2", rd("x1_0", 64, 1), v, ref)
    check("conv1_0.conv2 pooled", _read(model, "x1_0p", (B, 64, H >> 2, W >> 2)), em.pooled(v), F.max_pool2d(ref, 2))
    # conv after a pool: x1_0p -> x2_0a
    a = _read(model, "x1_0p", (B, 64, H >> 2, W >> 2))
    ap = em.act_from_planes(*[_read(model, "x1_0p#" + pl, (B, 64, H >> 2, W >> 2)) for pl in ("hi", "lo", "x8")])
    check("conv2_0.conv1", rd("x2_0a", 128, 2), em.conv_layer(ap, sd, "conv2_0.conv1"), fp32_layer(T(a), "conv2_0.conv1"))
    # deep conv (split-K plan at this size): x4_0a -> x4_0
    a = rd("x4_0a", 512, 4)
    check("conv4_0.conv2", rd("x4_0", 512, 4), em.conv_layer(act("x4_0a", 512, 4), sd, "conv4_0.conv2"), fp32_layer(T(a), "conv4_0.conv2"))
    # decoder conv1 with the fused upsample (level 1): cat([x1_0, up(x2_2)]) -> x1_3a
    sk, lo = rd("x1_0", 64, 1), rd("x2_2", 128, 2)
    v = em.decoder_conv1_layer(act("x1_0", 64, 1), act("x2_2", 128, 2), sd, "conv1_3.conv1", False)
    ref = fp32_layer(torch.cat([T(sk), F.interpolate(T(lo), scale_factor=2, mode="bilinear", align_corners=True)], 1), "conv1_3.conv1")
    check("conv1_3.conv1 + upsample", rd("x1_3a", 64, 1), v, ref)
    # decoder conv1 through the low-resolution GEMM (level 3): cat([x3_0, up(x4_0)]) -> x3_1a
    sk, lo = rd("x3_0", 256, 3), rd("x4_0", 512, 4)
    v = em.decoder_conv1_layer(act("x3_0", 256, 3), act("x4_0", 512, 4), sd, "conv3_1.conv1", True)
    ref = fp32_layer(torch.cat([T(sk), F.interpolate(T(lo), scale_factor=2, mode="bilinear", align_corners=True)], 1), "conv3_1.conv1")
    check("conv3_1.conv1 (low-resolution GEMM)", rd("x3_1a", 256, 3), v, ref)


# ---- SimpleUNet (reference src/models/simple_unet.py:94-128) in exact8: every conv through the wave-specialised
# kernel (the decoder's cat([up, enc]) as two full-resolution sources), the transposed convs on fp16 terms decoded from the 8-bit
# residual plane (csrc/convt2x2_mfma.h)

@pytest.mark.parametrize("tag", ["su_c7_32x48", "su_c3_64x40", "su_c7_256x256"])
def test_exact8_simple_unet_matches_golden(tag, torch_cuda, syn, oracle):
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    g = load_golden(tag)
    B, H, W, C = int(g["B"]), int(g["H"]), int(g["W"]), int(g["num_classes"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    sd = syn.make_simple_state_dict(C, 3, int(g["wseed"]))
    model = SimpleUNet(num_classes=C, num_channels=3, precision="exact8", max_batch=B, max_hw=(H, W)).to("cuda:0")
    model.load_state_dict(sd, strict=True)
    model.eval()
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    mask, logits = model.segment(x, return_logits=True)
    m_u8, l_u8 = model.segment(torch.from_numpy(frames).cuda(), return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(l_u8, logits) and torch.equal(m_u8, mask)          # the uint8 BGR entry computes the same bits
    lg, mk = logits.cpu().numpy(), mask.cpu().numpy()
    assert model.status() == 0
    if "logits" in g.files:
        gate(tag, lg, mk, g["logits"], g["mask"], oracle)
        for k in [f for f in g.files if f.startswith("t_")]:              # node by node: exact8-class (2^-13 of the largest value), not fp16-class
            got = model.debug_activation(k[2:], B, H, W)
            rel = float(np.abs(got - g[k]).max() / np.abs(g[k]).max())
            print(f"  {k[2:]}: {rel:.1e} of the largest value")
            assert rel < 1.5e-4, (k, rel)
    else:                                                                  # 256 x 256: the fixture holds every fourth logit, the mask and its ties
        err = float(np.abs(lg[:, :, ::4, ::4] - g["logits_sub4"]).max())
        ref = oracle.simple_unet_torch_forward(sd, syn.frames_to_chw_f32(frames))
        assert float(np.abs(ref[:, :, ::4, ::4] - g["logits_sub4"]).max()) < 1e-5      # the oracle is the fixture's reference
        gate(tag, lg, mk, ref, oracle.masks_from_logits(ref)[0], oracle)
        assert err < LOGIT_TOL


def test_exact8_simple_unet_random_shapes_and_batch_rows(torch_cuda, syn, oracle, monkeypatch):
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    monkeypatch.setenv("UNETPP_KSPLIT", "1")             # one launch plan for every batch size: rows must then agree bit for bit
    rng = np.random.default_rng(52001)
    for _ in range(6):
        C = int(rng.integers(1, 9)); B = int(rng.integers(2, 4))
        H = 8 * int(rng.integers(1, 17)); W = 8 * int(rng.integers(1, 17))
        sd = syn.make_simple_state_dict(C, 3, int(rng.integers(0, 50)))
        x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", int(rng.integers(0, 1000))))
        m = SimpleUNet(num_classes=C, num_channels=3, precision="exact8", max_batch=B, max_hw=(H, W)).to("cuda:0")
        m.load_state_dict(sd, strict=True)
        ref = oracle.simple_unet_torch_forward(sd, x)
        xt = torch.from_numpy(x).cuda()
        mask, logits = m.segment(xt, return_logits=True)
        one = m(xt[1:2])
        torch.cuda.synchronize()
        assert torch.equal(logits[1:2], one), (C, B, H, W)
        scale = max(1.0, float(np.abs(ref).max()))
        gate(f"simple C={C} B={B} {H}x{W}", logits.cpu().numpy() / scale, mask.cpu().numpy(), ref / scale, oracle.masks_from_logits(ref)[0], oracle)
