"""precision='fast' (include/unetpp.h UNETPP_PREC_FAST) held to its documented arithmetic LAYER BY LAYER: every stored tensor
of a forward is read back (unetpp_debug_read with debug_keep_intermediates) and every layer is emulated in float64
(oracle/fast_emulation.py) from the DEVICE'S OWN stored input, so nothing propagates.  The kernels under test are the ones only
this mode runs: conv3x3_bias_relu_kernel<1, ...> in every configuration launch_conv lists for P = 1 (csrc/conv3x3_mfma.h), its
fused-upsample loader, upsample2x_kernel<1>, convert_input_kernel<1>, head_generic_kernel<1> (csrc/aux_kernels.h) and
convt2x2_kernel<1> (csrc/convt2x2_mfma.h); and, for SimpleUNet's cat([up, enc]) convs, the same lock-step kernel with P = 2.

Criterion per element of a stored tensor, v the emulation's fp32 value and S = sum |a||w| 2^-k + |b|:
    |got - v| <= ulp_fp16(fp16(v)) / 2 + 4 gamma S
(the device stores fp16(v') of its own v', and a correct fp32 accumulation leaves v' within 4 gamma S of v: gamma is measured on
the reference alone by tests/test_fast_emulation_host.py, per kind of layer, fast_emulation.GAMMA; the factor 4 because the
MFMA's internal order is not the measured variant's), and at most 1 % of a layer's elements may differ from fp16(v) at all (the
reference's own variant differs in 0.1 % or less).  fp32 outputs (logits) get the 4 gamma S term only.  A tap dropped at a seam, a
weight off in one column, a second rounding or a wrong pool row all break the first condition by a factor of 130 to 160000
(tests/test_fast_emulation_host.py, negative controls) while staying inside the 5e-2 the end-to-end tests ask for.

Measured on the MI355X (DESIGN.md §3 has the table): every conv, pooled copy and transposed conv uses 0.01-0.19 of its
allowance 4 gamma S, conv0_4.conv1 with the loader's interpolation 0.04-0.09, the heads 0.17-0.43, the fused head 0.01; the `u`
tensors equal the emulation bit for bit at every shape; 0.01-0.16 % of a conv layer's elements differ from fp16(v) (the
reference's own variant: 0.02-0.09 %).
End to end, mean |device - emulation| / mean |emulation - oracle|: 0.86 at 2x64x96, 0.83 at 2x128x160 (exact8, layer by
layer: 1/22 .. 1/90) -- after 18 layers the 0.02-0.15 % of roundings that flip per layer have spread, and two correct
implementations of 'fast' are as far from each other as from the reference; which is why the layers are judged one by one.
Run on the GPU box:  python -m pytest tests -m gpu"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NB = (32, 64, 128, 256, 512)
SB = (64, 128, 256, 512)
MAX_SHARE = 0.01


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def fe():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import fast_emulation
    return fast_emulation


def make_nested(sd, B, hw, precision="fast"):
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=True, precision=precision, max_batch=B, max_hw=hw).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    return m.eval()


def make_simple(sd, C, B, hw, precision):
    from unet_amd.nested_unet import SimpleUNet
    m = SimpleUNet(num_classes=C, num_channels=3, precision=precision, max_batch=B, max_hw=hw).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    return m.eval()


def _shape(name, B, H, W):
    """[B, C, h, w] of an engine tensor from its name (csrc/unetpp_abi.hip build_nested / build_simple)"""
    base = name.split("#")[0]
    if base == "in8":
        return (B, 8, H, W)
    if base[0] == "x":
        l = int(base[1])
        c, lvl = (NB[l + 1], l) if base.endswith("u") else (NB[l], l + 1) if base.endswith("p") else (NB[l], l)
    elif base.startswith("up"):
        l = int(base[2]) - 1
        c, lvl = SB[l], l
    else:
        l = int(base[3]) - 1
        c, lvl = SB[l], l + 1 if base.endswith("p") else l
    return (B, c, H >> lvl, W >> lvl)


class Reader:
    """unetpp_debug_read of any stored tensor of the last forward, as float64 torch tensors (cached)"""

    def __init__(self, model, B, H, W, fe):
        self.model, self.dims, self.fe, self.cache = model, (B, H, W), fe, {}

    def np(self, name):
        from unet_amd import _lib
        out = np.empty(_shape(name, *self.dims), dtype=np.float32)
        n = _lib.load().unetpp_debug_read(self.model._handle, name.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
        assert n == out.size, (name, n, out.size, self.model._err(int(n)) if n < 0 else "")
        return out

    def __call__(self, name):
        if name not in self.cache:
            self.cache[name] = self.fe._t(self.np(name))
        return self.cache[name]


class Table:
    """one line per layer: allowance used, share of differing elements; asserts at the end so that the whole table prints"""

    def __init__(self, fe, title):
        self.fe, self.rows, self.title = fe, [], title

    def add(self, tag, kind, got, v, S, rounded=True, gamma=None, frames=None):
        if frames is not None:
            got = got[frames]
        g = self.fe.GAMMA[kind] if gamma is None else gamma
        ratio, share = self.fe.layer_check(got, v, S, g, rounded)
        self.rows.append((tag, kind, g, ratio, share))

    def finish(self):
        print(f"\n{self.title}\n  layer | kind | gamma | allowance used | elements that differ from the emulation")
        for tag, kind, g, ratio, share in self.rows:
            print(f"  {tag:24s} {kind:6s} {g:.1e}  {ratio:6.3f}  {share:.4%}")
        bad = [r for r in self.rows if not (r[3] <= 1.0 and r[4] <= MAX_SHARE)]
        assert not bad, bad


def walk_nested(fe, rd, sd, x_in, tab, prefix=""):
    """every layer of the NestedUNet forward in 'fast' (debug_keep_intermediates on: the head runs unfused), each from the
    device's own stored input"""
    import torch
    emu_in = fe.input_plane(x_in)
    assert torch.equal(rd("in8"), emu_in), "in8: convert_input_kernel<1> must give the emulation's bits"
    cur = "in8"
    for l in range(5):
        tn, cn = f"x{l}_0", f"conv{l}_0"
        tab.add(prefix + cn + ".conv1", "conv", rd(tn + "a"), *fe.conv(rd(cur), *fe._fold(sd, cn + ".conv1")))
        v, S = fe.conv(rd(tn + "a"), *fe._fold(sd, cn + ".conv2"))
        tab.add(prefix + cn + ".conv2", "conv", rd(tn), v, S)
        if l < 4:
            tab.add(prefix + cn + ".conv2 pooled", "conv", rd(tn + "p"), *fe.pooled(v, S=S))
            cur = tn + "p"
    low = "x4_0"
    for l in (3, 2, 1, 0):
        tn, cn = f"x{l}_{4 - l}", f"conv{l}_{4 - l}"
        w1, b1 = fe._fold(sd, cn + ".conv1")
        if l == 0:
            tab.add(prefix + cn + ".conv1 + up", "conv", rd(tn + "a"), *fe.decoder_conv1_upf(rd("x0_0"), rd(low), w1, b1))
        else:
            tab.add(prefix + tn + "u", "up", rd(tn + "u"), *fe.upsample(rd(low)))
            tab.add(prefix + cn + ".conv1", "conv", rd(tn + "a"), *fe.conv(torch.cat([rd(f"x{l}_0"), rd(tn + "u")], 1), w1, b1))
        tab.add(prefix + cn + ".conv2", "conv", rd(tn), *fe.conv(rd(tn + "a"), *fe._fold(sd, cn + ".conv2")))
        low = tn


@pytest.fixture(scope="module")
def base(torch_cuda, fe, syn):
    """2x64x96 (split rows and columns, W no multiple of 32 at levels 1-2): one engine, one kept forward, shared"""
    torch = torch_cuda
    B, H, W = 2, 64, 96
    sd = syn.make_state_dict(3, 3, True, 2)
    frames = syn.make_frames_u8(B, H, W, "smooth", 7)
    x = syn.frames_to_chw_f32(frames)
    model = make_nested(sd, B, (H, W))
    xt = torch.from_numpy(x).cuda()
    fused = model(xt)                                   # the product path: head fused into conv0_4.conv2
    torch.cuda.synchronize()
    x0_4a = Reader(model, B, H, W, fe)("x0_4a")
    model.debug_keep_intermediates(True)
    model.profile(True)
    unfused = model(xt)
    torch.cuda.synchronize()
    names = [r[0] for r in model.profile_read()]
    model.profile(False)
    rd = Reader(model, B, H, W, fe)
    for l in range(5):                                  # every stored tensor now: later calls on the engine cannot change what is read
        for sfx in ("a", "") + (("p",) if l < 4 else ()):
            rd(f"x{l}_0{sfx}")
        if l < 4:
            for sfx in ("a", "") + (("u",) if l else ()):
                rd(f"x{l}_{4 - l}{sfx}")
    rd("in8")
    return dict(model=model, sd=sd, frames=frames, x=x, xt=xt, dims=(B, H, W), fused=fused.cpu().numpy(), x0_4a=x0_4a,
                unfused=unfused.cpu().numpy(), names=names, rd=rd)


def test_every_layer_at_2x64x96(base, fe):
    """conv0_0.conv1 (C = 8 tensor, KC = 16), conv1_0.conv2 + pooled copy (KC = 32, NW = 2), the convs after a pool, conv2_0 /
    conv3_0 / conv4_0 (NW = 4), conv0_4.conv1 (UPF loader), the two-source convs and the three `u` tensors, the unfused head
    (head_generic_kernel<1> on the stored x0_4) -- and every other layer of the forward"""
    tab = Table(fe, "fast, 2x64x96, every layer from the device's own stored input")
    walk_nested(fe, base["rd"], base["sd"], base["x"], tab)
    tab.add("final (head_generic<1>)", "head", base["unfused"], *fe.head_generic(base["rd"]("x0_4"), *fe._head_wb(base["sd"])), rounded=False)
    tab.finish()
    # small launches take the 8-row tiles (MW = 1) wherever nothing is fused: 2 x 2 x 2 tiles at level 1
    assert "conv1_3.conv2|conv3x3_bias_relu_kernel<1, 32, 2, 1, 8, false, false, false>" in base["names"], base["names"]
    assert "conv0_4.conv1+up|conv3x3_bias_relu_kernel<1, 16, 1, 2, 8, false, false, true>" in base["names"], base["names"]
    assert sum("|upsample2x_kernel<1>" in n for n in base["names"]) == 3 and "final+argmax|head_generic_kernel<1>" in base["names"]


def test_input_plane_from_u8_frames(base, fe, torch_cuda):
    """in8 from uint8 BGR frames: fp16(b / 255) with the division correctly rounded, channels reversed -- the emulation's bits
    (an engine of the test's own: the shared one keeps the forward the other tests read)"""
    torch = torch_cuda
    B, H, W = base["dims"]
    model = make_nested(base["sd"], B, (H, W))
    lg = model(torch.from_numpy(base["frames"]).cuda())
    torch.cuda.synchronize()
    assert torch.equal(Reader(model, B, H, W, fe)("in8"), fe.input_plane(base["frames"]))
    assert np.array_equal(lg.cpu().numpy(), base["fused"])


def test_fused_head_logits_in_fp32(base, fe):
    """conv0_4.conv2 + the fused head against the emulated fp32 logits: nothing is rounded to fp16 between the two, so the
    bound has the fp32 terms only -- the conv's 4 gamma S carried through |w_head|, plus the head's own."""
    import torch
    sd = base["sd"]
    v, Sc = fe.conv(base["x0_4a"], *fe._fold(sd, "conv0_4.conv2"))
    wf, bf = fe._head_wb(sd)
    lg, _ = fe.head_fused(v, wf, bf)
    S = torch.einsum("bchw,kc->bkhw", Sc, wf.reshape(wf.shape[0], -1).abs()) + bf.abs()[None, :, None, None]
    tab = Table(fe, "fast, 2x64x96, fused head")
    tab.add("conv0_4.conv2 + final", "head", base["fused"], lg, S, rounded=False, gamma=fe.GAMMA["conv"] + fe.GAMMA["head"])
    tab.finish()
    assert "conv0_4.conv2" in "".join(base["names"])


def test_deep_supervision_heads_on_stored_nodes(base, fe, torch_cuda):
    """head_generic_kernel<1> on the stored nodes x1_3, x2_2, x3_1 (logits only), then ds_upsample_kernel's one fp32 bilinear
    step (ATen's rule, which tests/test_gpu_deep_supervision.py pins on F.interpolate in float32): against the emulated head,
    interpolated the same way.  Bound: the head's 4 gamma S, interpolated, plus the interpolation's own four fp32 roundings
    of values up to the largest low-resolution logit, should ATen take them in another order."""
    import torch.nn.functional as F
    torch = torch_cuda
    model, sd, (B, H, W) = base["model"], base["sd"], base["dims"]
    outs = model.forward_deep_supervision(base["xt"])
    torch.cuda.synchronize()
    up = lambda t: F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True)
    print()
    for k, head, node in ((1, "ds1_3", "x1_3"), (2, "ds2_2", "x2_2"), (3, "ds3_1", "x3_1")):
        low, S = fe.head_generic(base["rd"](node), *fe._head_wb(sd, head))
        bound = 4 * fe.GAMMA["head"] * up(S) + 4 * 2.0 ** -24 * float(low.abs().max())
        dev = (fe._t(outs[k].cpu().numpy()) - up(low.float()).double()).abs()
        ratio = float((dev / bound).max())
        print(f"  out{k} ({head} on the stored {node}): allowance used = {ratio:.3f}, max deviation {float(dev.max()):.2e}")
        assert ratio <= 1.0, (k, ratio)


@pytest.mark.parametrize("B,H,W", [(3, 16, 80), (2, 80, 16), (1, 32, 1056)])
def test_every_layer_at_edge_shapes(B, H, W, fe, syn, torch_cuda):
    """3x16x80 and 2x80x16: a single row / column of tiles, 2.5 tiles along the other axis.  1x32x1056: upsample2x_kernel crosses
    two 256-column segment seams at level 1 (W = 528) with permuted row pairs (H/2 = 8), against H/2 = 4 and 2 at levels 2-3."""
    torch = torch_cuda
    sd = syn.make_state_dict(3, 3, True, 2)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 100 + H + W))
    model = make_nested(sd, B, (H, W))
    model.debug_keep_intermediates(True)
    lg = model(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    rd = Reader(model, B, H, W, fe)
    tab = Table(fe, f"fast, {B}x{H}x{W}, every layer from the device's own stored input")
    walk_nested(fe, rd, sd, x, tab)
    tab.add("final (head_generic<1>)", "head", lg.cpu().numpy(), *fe.head_generic(rd("x0_4"), *fe._head_wb(sd)), rounded=False)
    tab.finish()
    assert model.status() == 0


def test_interpolation_weights_at_level1_height_128(fe, syn, torch_cuda):
    """1x256x48: the `u` tensors where the weight rule matters -- source coordinates up to 63 at level 1 (x1_3u is 128 rows) and
    up to 127 in the loader of level 0.  A weight taken from the rounded coordinate instead of the single fma is off by up to
    2^-24 of the coordinate there, five times the allowance of a `u` tensor."""
    torch = torch_cuda
    B, H, W = 1, 256, 48
    sd = syn.make_state_dict(3, 3, True, 2)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 13))
    model = make_nested(sd, B, (H, W))
    model.debug_keep_intermediates(True)
    model(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    rd = Reader(model, B, H, W, fe)
    tab = Table(fe, f"fast, {B}x{H}x{W}, the interpolated tensors")
    for l, low in ((3, "x4_0"), (2, "x3_1"), (1, "x2_2")):
        tab.add(f"x{l}_{4 - l}u", "up", rd(f"x{l}_{4 - l}u"), *fe.upsample(rd(low)))
    tab.add("conv0_4.conv1 + up", "conv", rd("x0_4a"), *fe.decoder_conv1_upf(rd("x0_0"), rd("x1_3"), *fe._fold(sd, "conv0_4.conv1")))
    tab.finish()
    assert model.status() == 0


def test_16_row_tiles_at_8x256x256(fe, syn, torch_cuda):
    """conv1_3.conv2 at 8x256x256: 8 x 4 x 8 tiles of 16 x 32 pixels reach the CU count, so the 16-row variant (MW = 2) runs where
    2x64x96 ran the 8-row one.  Frames 0 and 7 are emulated."""
    torch = torch_cuda
    B, H, W = 8, 256, 256
    sd = syn.make_state_dict(3, 3, True, 2)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 11))
    model = make_nested(sd, B, (H, W))
    model.debug_keep_intermediates(True)
    xt = torch.from_numpy(x).cuda()
    model(xt)                                           # creates the engine
    model.profile(True)
    model(xt)
    torch.cuda.synchronize()
    names = [r[0] for r in model.profile_read()]
    assert "conv1_3.conv2|conv3x3_bias_relu_kernel<1, 32, 2, 2, 8, false, false, false>" in names, names
    rd = Reader(model, B, H, W, fe)
    tab = Table(fe, "fast, 8x256x256, conv1_3.conv2 with 16-row tiles, frames 0 and 7")
    tab.add("conv1_3.conv2 (MW = 2)", "conv", rd("x1_3"), *fe.conv(rd("x1_3a")[[0, 7]], *fe._fold(sd, "conv1_3.conv2")), frames=[0, 7])
    tab.finish()
    assert model.status() == 0


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (2, 128, 160)])
def test_end_to_end_against_the_emulation(B, H, W, base, fe, syn, oracle, torch_cuda):
    """Whole network: the device may be at most twice as far from the oracle as the documented arithmetic is (the form of
    tests/test_gpu_value_range.py C.2), plus the head's fp32 allowance.  The ratio mean|device - emulation| / mean|emulation -
    oracle| is printed, not asserted (module docstring)."""
    torch = torch_cuda
    sd = base["sd"]
    if (B, H, W) == base["dims"]:
        x, dev = base["x"], base["fused"]
    else:
        x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 7))
        model = make_nested(sd, B, (H, W))
        dev = model(torch.from_numpy(x).cuda()).cpu().numpy()
        assert model.status() == 0
    ref = oracle.torch_forward(sd, x)
    emu, nd = fe.fast_forward(sd, x, return_nodes=True)
    _, S = fe.head_generic(fe._t(nd["x0_4"]), *fe._head_wb(sd))
    err, emu_err = float(np.abs(dev - ref).max()), float(np.abs(emu - ref).max())
    ratio = float(np.abs(dev - emu).mean() / np.abs(emu - ref).mean())
    print(f"\nfast {B}x{H}x{W}: max|device - oracle| = {err:.3e}, max|emulation - oracle| = {emu_err:.3e}, max|device - emulation| = "
          f"{float(np.abs(dev - emu).max()):.3e}, mean|device - emulation| / mean|emulation - oracle| = {ratio:.3f}")
    assert err <= 2 * emu_err + 4 * fe.GAMMA["head"] * float(S.max())


# ---- SimpleUNet (reference src/models/simple_unet.py:94-128): the P = 1 transposed conv, cat([up, enc]) through the two-source loader

def test_simple_unet_every_layer_fast(fe, syn, torch_cuda):
    torch = torch_cuda
    C, B, H, W = 7, 2, 32, 48
    sd = syn.make_simple_state_dict(C, 3, 3)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 7))
    model = make_simple(sd, C, B, (H, W), "fast")
    model.debug_keep_intermediates(True)
    lg = model(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    rd = Reader(model, B, H, W, fe)
    assert torch.equal(rd("in8"), fe.input_plane(x))
    tab = Table(fe, f"SimpleUNet fast, {B}x{H}x{W}, every layer from the device's own stored input")
    cur = "in8"
    for l in range(1, 5):
        tn = f"enc{l}"
        tab.add(tn + ".0", "conv", rd(tn + "a"), *fe.conv(rd(cur), *fe._plain(sd, tn + ".0")))
        v, S = fe.conv(rd(tn + "a"), *fe._plain(sd, tn + ".2"))
        tab.add(tn + ".2", "conv", rd(tn), v, S)
        if l < 4:
            tab.add(tn + ".2 pooled", "conv", rd(tn + "p"), *fe.pooled(v, S=S))
            cur = tn + "p"
    prev = "enc4"
    for l in (3, 2, 1):
        tab.add(f"up{l} (convt2x2<1>)", "convt", rd(f"up{l}t"), *fe.convt(rd(prev), *fe._plain(sd, f"up{l}")))
        tn = f"dec{l}"
        tab.add(tn + ".0 (cat)", "conv", rd(tn + "a"), *fe.conv(torch.cat([rd(f"up{l}t"), rd(f"enc{l}")], 1), *fe._plain(sd, tn + ".0")))
        tab.add(tn + ".2", "conv", rd(tn), *fe.conv(rd(tn + "a"), *fe._plain(sd, tn + ".2")))
        prev = tn
    tab.add("final (head_generic<1>)", "head", lg.cpu().numpy(), *fe.head_generic(rd("dec1"), *fe._head_wb(sd)), rounded=False)
    tab.finish()
    assert model.status() == 0


def test_simple_unet_up3_and_dec3_exact(fe, syn, torch_cuda):
    """'exact': up3 (convt2x2_kernel<2>) and dec3.0 -- the one conv of 'exact' that runs in the lock-step kernel (P = 2, two
    full-resolution sources) -- from the device's own stored planes, with exact_emulation's three-term product, at the bar the
    suite holds 'exact' to (2e-5 of the largest value; measured figures are printed)."""
    import torch.nn.functional as F
    import exact_emulation as ee
    torch = torch_cuda
    C, B, H, W = 7, 2, 32, 48
    sd = syn.make_simple_state_dict(C, 3, 3)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 7))
    model = make_simple(sd, C, B, (H, W), "exact")
    model.debug_keep_intermediates(True)
    xt = torch.from_numpy(x).cuda()
    model(xt)                                           # creates the engine
    model.profile(True)
    model(xt)
    torch.cuda.synchronize()
    names = [r[0] for r in model.profile_read()]
    assert any(n.startswith("dec3.0|conv3x3_bias_relu_kernel<2, 16, 2, ") for n in names), names
    rd = Reader(model, B, H, W, fe)
    act = lambda n: ee.act_from_planes(rd(n + "#hi"), rd(n + "#lo"))
    # dec3.0: cat([up3t, enc3]) -> dec3a
    w, b = fe._plain(sd, "dec3.0")
    emu = ee.Act(ee._conv(ee._cat([act("up3t"), act("enc3")]), w, b)).value
    err = float((rd("dec3a") - emu).abs().max()); top = float(emu.abs().max())
    print(f"\nSimpleUNet exact 2x32x48 dec3.0 (lock-step P = 2): max|device - emulation| = {err:.2e} of values up to {top:.2f}")
    assert err <= 2e-5 * max(1.0, top)
    # up3: enc4 -> up3t, hi wh + lo wh + hi wl per output channel's power-of-two scale
    w, b = fe._plain(sd, "up3")
    m = w.abs().amax(dim=(0, 2, 3))
    k = 14 - (torch.floor(torch.log2(m)) + 1)
    ws = w * (2.0 ** k)[None, :, None, None]
    wh = fe._f16(ws); wl = fe._f16(ws - wh)
    a = act("enc4")
    ct = lambda p, q: F.conv_transpose2d(p, q, stride=2)
    acc = ct(a.h, wh) + ct(a.l, wh) + ct(a.h, wl)
    emu = ee.Act(fe._f32(acc * (2.0 ** -k)[None, :, None, None] + b[None, :, None, None])).value
    err = float((rd("up3t") - emu).abs().max()); top = float(emu.abs().max())
    print(f"SimpleUNet exact 2x32x48 up3 (convt2x2<2>): max|device - emulation| = {err:.2e} of values up to {top:.2f}")
    assert err <= 2e-5 * max(1.0, top)
    assert model.status() == 0


def test_exact8_input_tensor_reads_back_its_own_planes(fe, syn, torch_cuda):
    """SimpleUNet in exact8 materialises in8 as a 32-byte record of 8 channels, {hi x 8}{lo8 c0-3, x8 c0-3, 0, 0}:
    unetpp_debug_read must decode THAT layout (it used to read the 8-bit planes 32 bytes in, i.e. from the next pixel, and past
    the tensor for the last one).  in8, in8#hi, in8#lo and in8#x8 equal the host's split of the input."""
    import exact8_emulation as e8
    torch = torch_cuda
    C, B, H, W = 3, 2, 16, 24
    sd = syn.make_simple_state_dict(C, 3, 3)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "uniform", 5))
    model = make_simple(sd, C, B, (H, W), "exact8")
    model(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    rd = Reader(model, B, H, W, fe)
    a = e8.Act(torch.cat([fe._t(x), torch.zeros(B, 5, H, W, dtype=torch.float64)], 1))
    assert torch.equal(rd("in8#hi"), a.h)
    assert torch.equal(rd("in8#lo"), a.l8)
    assert torch.equal(rd("in8#x8"), a.x8)
    assert torch.equal(rd("in8"), fe._f32(a.value))
    assert float(a.l8.abs().max()) > 0 and float(a.x8.abs().max()) > 0 and model.status() == 0
