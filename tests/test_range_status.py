"""The engine stores activations as fp16 planes; the fp32 reference (src/models/unetpp.py:17-26,
src/models/simple_unet.py:94-128) has no 65504 ceiling and propagates NaN.  Values that do not fit are never
narrowed silently: the kernel sets a sticky flag (include/unetpp.h unetpp_status).  Also: BatchNorm statistics of
the kind only trained checkpoints have (tiny running_var, negative / zero gamma) must fold correctly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OVERFLOW, NAN = 1, 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


def test_trained_like_bn_statistics_match_oracle(torch_cuda, syn, oracle):
    """(c) running_var = 1e-8 on near-dead channels, gamma < 0, gamma = 0, large gamma: parity with the oracle, no flag."""
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    sd = syn.make_trained_like_state_dict(3, 3, True, 2)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(2, 64, 96, "smooth", 7))
    ref, inter = oracle.torch_forward(sd, x, return_intermediates=True)
    ref_mask, _, _ = oracle.masks_from_logits(ref)
    m = NestedUNet(3, max_batch=2, max_hw=(64, 96)).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    m.debug_keep_intermediates(True)
    logits = m(torch.from_numpy(x).cuda()).cpu().numpy()
    for name in ("x0_0", "x2_0", "x4_0", "x2_2", "x0_4"):
        got = m.debug_activation(name, 2, 64, 96)
        scale = max(1.0, float(np.abs(inter[name]).max()))
        np.testing.assert_allclose(got, inter[name], rtol=0, atol=2e-5 * scale, err_msg=name)
    m.debug_keep_intermediates(False)
    mask = m.segment(torch.from_numpy(x).cuda()).cpu().numpy()
    err = float(np.abs(logits - ref).max())
    print(f"trained-like BN: max|dlogit|={err:.3e}, logits in [{ref.min():.2f},{ref.max():.2f}]")
    assert err < 1e-3 and err < 2e-5 * max(1.0, float(np.abs(ref).max()))
    flips = mask != ref_mask
    assert not (flips & (oracle.top2_margin(ref) > 2 * err + 1e-7)).any()
    assert m.status() == 0


def test_simple_unet_overflow_sets_flag(torch_cuda, syn, oracle):
    """(a) SimpleUNet has no BatchNorm: a large-gain checkpoint drives activations past the fp16 maximum."""
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    x = syn.frames_to_chw_f32(syn.make_frames_u8(1, 64, 64, "smooth", 7))
    xt = torch.from_numpy(x).cuda()

    def scaled(gain):
        sd = syn.make_simple_state_dict(7, 3, 0)
        for k in ("enc1.0.weight", "enc1.0.bias"):
            sd[k] = sd[k] * np.float32(gain)
        return sd

    # activations of a few thousand: representable, must match the oracle (relative to their size) and raise no flag
    sd = scaled(1000.0)
    ref, inter = oracle.simple_unet_torch_forward(sd, x, return_intermediates=True)
    assert 1e3 < max(float(np.abs(v).max()) for v in inter.values()) < 6e4
    m = SimpleUNet(7, 3, max_batch=1, max_hw=(64, 64)).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    logits = m(xt).cpu().numpy()
    assert float(np.abs(logits - ref).max()) < 2e-5 * float(np.abs(ref).max())
    assert m.status() == 0

    # the same net 40x louder: enc1 exceeds 65504 -> clamped -> flagged (and kept flagged until cleared)
    sd = scaled(40000.0)
    _, inter = oracle.simple_unet_torch_forward(sd, x, return_intermediates=True)
    assert float(np.abs(inter["enc1"]).max()) > 65504
    m.load_state_dict(sd, strict=True)
    m(xt)
    assert m.status() & OVERFLOW
    assert m.status(clear=True) & OVERFLOW
    assert m.status() == 0
    strict = SimpleUNet(7, 3, max_batch=1, max_hw=(64, 64), check_range=True).to("cuda:0")
    strict.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="value range"):
        strict(xt)


ENGINE_KINDS = [(arch, prec) for arch in ("nested", "simple") for prec in ("exact", "exact8", "fast")]


def _quiet_first_conv(syn, arch):
    """(model class, classes, state dict whose first conv's weight is multiplied by 2^-10): an input of +-65504 then leaves
    every activation far inside the range, so the input alone decides the flags"""
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    if arch == "nested":
        sd, key, cls, C = syn.make_state_dict(3, 3, True, 2), "conv0_0.conv1.weight", NestedUNet, 3
    else:
        sd, key, cls, C = syn.make_simple_state_dict(7, 3, 0), "enc1.0.weight", SimpleUNet, 7
    sd[key] = sd[key] * np.float32(2.0 ** -10)
    return cls, C, sd


@pytest.mark.parametrize("arch,prec", ENGINE_KINDS)
def test_nan_and_huge_input_set_flags(arch, prec, torch_cuda, syn, oracle):
    """(b) a NaN pixel / a float32 input at and beyond the fp16 range, in the six engine kinds (the four pieces of code that
    ingest the input: conv3x3_ws.h's patch loader, convert_input_kernel<1>, <2> and <2, true>).  +-65504 is inside the range:
    no flag, parity.  Beyond it the header promises a clamp and the OVERFLOW flag: the outputs are those of the tensor clamped
    on the host, bit for bit.  A NaN raises NAN and reaches no output."""
    import os
    import sys
    from conftest import ROOT
    from test_input_domain_host import EXACT_BAR, FAST_TOL, NORTH_STAR, bits_equal, scale_of
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import exact8_emulation as em8
    import fast_emulation as fe
    torch = torch_cuda
    B, H, W = 1, 32, 48
    cls, C, sd = _quiet_first_conv(syn, arch)
    kw = dict(precision=prec, max_batch=B, max_hw=(H, W))
    m = cls(C, **kw).to("cuda:0")
    m.load_state_dict(sd, strict=True)

    def run(a):
        mask, logits = m.segment(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda(), return_logits=True)
        torch.cuda.synchronize()
        return logits.cpu().numpy(), mask.cpu().numpy()

    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 3))
    run(x)
    assert m.status() == 0

    # exactly +-65504 at the corners and on the first block's tile seams: representable, so no flag, and parity as for any input
    xi = syn.make_inputs_f32("impulses", B, H, W, 3) * np.float32(65504.0)
    assert float(np.abs(xi).max()) == 65504.0 and (xi < 0).any() and (xi > 0).any()
    fwd = oracle.torch_forward if arch == "nested" else oracle.simple_unet_torch_forward
    ref, inter = fwd(sd, xi, return_intermediates=True)
    assert max(float(np.abs(v).max()) for v in inter.values()) < 2.0 ** 15      # the input alone is large
    s = scale_of(ref)
    cap = EXACT_BAR[arch] * s
    if prec == "exact8":
        cap = min(2 * float(np.abs(em8.exact8_forward(sd, xi) - ref).max()) + cap, NORTH_STAR * s) if arch == "nested" else NORTH_STAR * s
    elif prec == "fast":
        emu = fe.fast_forward(sd, xi) if arch == "nested" else fe.fast_simple_forward(sd, xi)
        cap = min(2 * float(np.abs(emu - ref).max()) + cap, FAST_TOL * s)
    lg, mk = run(xi)
    err = float(np.abs(lg - ref).max())
    print(f"{arch} {prec}: +-65504 impulses, max|dlogit| / s = {err / s:.2e} (cap {cap / s:.2e}), s = {s:.3g}")
    assert m.status() == 0
    assert np.isfinite(lg).all() and err <= cap
    assert not ((mk != oracle.masks_from_logits(ref)[0]) & (oracle.top2_margin(ref) > 2 * err + 1e-7)).any()

    # a NaN: flagged, and every output stays finite -- also where only a neighbouring tile's halo reads the pixel a second time
    for pos in ((0, 1, 7, 9), (0, 0, 16, 32)):
        xn = x.copy(); xn[pos] = np.float32("nan")
        lg, _ = run(xn)
        assert m.status(clear=True) & NAN, pos
        assert np.isfinite(lg).all(), pos
        assert m.status() == 0

    # beyond the range: OVERFLOW (and not NAN), results of the clamped tensor, bit for bit
    for pos, v in (((0, 2, 20, 30), 1.0e6), ((0, 1, 16, 32), -1.0e6), ((0, 0, 0, 0), float("inf")), ((0, 2, H - 1, W - 1), float("-inf"))):
        xb = x.copy(); xb[pos] = np.float32(v)
        lg, mk = run(xb)
        st = m.status(clear=True)
        assert st & OVERFLOW and not st & NAN, (v, st)
        lc, mc = run(np.clip(xb, np.float32(-65504.0), np.float32(65504.0)))
        assert m.status() == 0, v
        assert bits_equal(lg, lc) and np.array_equal(mk, mc), v
    # the first float32 value that does not round to an fp16 number (values between 65504 and 65520 are left unspecified)
    for v in (65520.0, -65520.0):
        xb = x.copy(); xb[0, 1, 15, 31] = np.float32(v)
        run(xb)
        assert m.status(clear=True) & OVERFLOW, v

    run(x)                                         # sticky, not stuck: clean again after the clear
    assert m.status() == 0
    # uint8 frames cannot leave the range
    run(torch.from_numpy(syn.make_frames_u8(B, H, W, "uniform", 4)).cuda())
    assert m.status() == 0

    strict = cls(C, check_range=True, **kw).to("cuda:0")
    strict.load_state_dict(sd, strict=True)
    strict(torch.from_numpy(x).cuda())
    for v in (1.0e6, float("nan")):
        xb = x.copy(); xb[0, 2, 20, 30] = np.float32(v)
        with pytest.raises(RuntimeError, match="value range"):
            strict(torch.from_numpy(xb).cuda())
    strict(torch.from_numpy(x).cuda())             # the raise cleared the flags


def test_non_finite_weights_set_flag_at_load(torch_cuda, syn):
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    sd = syn.make_state_dict(3, 3, True, 2)
    sd["conv2_0.conv1.weight"] = sd["conv2_0.conv1.weight"].copy()
    sd["conv2_0.conv1.weight"][5, 7, 1, 1] = np.float32("nan")
    m = NestedUNet(3, max_batch=1, max_hw=(32, 32)).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    m.segment(torch.from_numpy(syn.frames_to_chw_f32(syn.make_frames_u8(1, 32, 32, "smooth", 3))).cuda())
    assert m.status(clear=True) & NAN
    sd = syn.make_state_dict(3, 3, True, 2)
    sd["conv0_4.bn2.bias"] = sd["conv0_4.bn2.bias"].copy()
    sd["conv0_4.bn2.bias"][3] = np.float32("inf")
    m.load_state_dict(sd, strict=True)
    assert m.status(clear=True) & NAN
    m.load_state_dict(syn.make_state_dict(3, 3, True, 2), strict=True)
    assert m.status() == 0
