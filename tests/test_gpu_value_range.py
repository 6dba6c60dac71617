"""The exact modes across the activation and logit value range (device side; tests/test_value_range_host.py is the CPU side).

Every other parity test runs on checkpoints whose stored activations sit around 1 and whose logits sit in +-3.  The engine stores
activations as fp16 planes (`exact`: hi + lo, `exact8`: hi + two e5m2 planes), which have a window: 65504 at the top, and at the
bottom the `lo` plane goes subnormal as soon as |x| < 0.25.  Where a tensor sits is arbitrary in the fp32 reference (a block's
BatchNorm scale and its consumers' weights trade any power of two, bit for bit: `synthetic.rescale_state_dict`, proven on the
CPU), so here ONE tensor at a time is moved through the window -- the nine nodes and the nine inner tensors of NestedUNet --
and the device is held to `oracle.torch_forward` on the rescaled checkpoint:

  C.1  inside the window (from the k the float64 emulation of `exact` derives, test_value_range_host.window_low, up to k_hi, at
       which the tensor peaks at 29,000 ... 59,000): logits at the bars the suite holds the modes to at these sizes (`exact`
       2e-5; `exact8` 1e-3 and mask flips only at near-ties), the tensor read back within 2e-5 of its largest value in `exact`
       (`exact8`: 3e-4, the bar tests/test_gpu_exact8.py holds that mode's stored nodes to -- its second plane carries 2 mantissa
       bits, 2^-14 of the value, so 2e-5 is not a property of the format; the figure against 2e-5 is printed), no status flag.
  C.2  below the window, down to the k at which the emulation itself reaches 1e-3 (`exact`): the device may lose at most twice
       what the documented arithmetic loses (+ 2e-5): fp32 summation order, DESIGN.md §2.
  C.3  over the top (k_hi + 2; k_hi + 1 where that leaves no untouched 32-pixel segment): OVERFLOW set, sticky, clean after a
       clear and an in-range forward, never NAN; the stored tensor and its pooled copy are exactly 65504 where the reference
       exceeds it and close to the reference where it does not; in `exact8` the lo8 plane of a clamped element is 0 and its x8
       plane e5m2(65504 / 8).  `exact` is held to the margins 1e-4 and the tolerance 2e-5 x 65504; `exact8` and `fast` (lock-step
       epilogue) to their own node bars scaled by the tensor's largest value (_c3_bounds says why).
  C.4  the logits scaled by 2^k (this changes the function): `exact` inside 1e-3 absolute up to +-70; `exact8` within twice its
       committed emulation; probabilities, masks and the three class rules where `exp` saturates.

Shapes: 2x64x96 (split-K plan at level 4, low-resolution GEMM at levels 2-3) for every site; 2x512x512 (persistent multi-tile
schedule) for x0_0, x1_0, x1_3a, x3_1a in C.1 and C.3.  C.2 stays at 2x64x96: its bound needs the float64 emulation of the same
case, which takes 45 s per case at 512x512.

Negative controls, run once on the CPU against the emulation (tests/test_value_range_host.py::
test_negative_controls_against_the_emulation): an emulation that drops the lo plane of the site, and one that clamps at 32768
instead of 65504, each fail C.1 at k = k_hi; one that stores the pooled tensor unclamped fails C.3.

Run on the GPU box:  python -m pytest tests -m gpu"""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_value_range_host import (EXACT_SMALL_BAR, F16_MAX, LOGIT_CASES, LOGIT_SHAPES, NB, NORTH_STAR, RULES, below_window,
                                   boundary_distance, clamp_check, k_hi, nested_case, reference_tensors, softmax64, window_low)

sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

OVERFLOW, NAN = 1, 2
X8_NODE_BAR = 3e-4                        # tests/test_gpu_exact8.py: a stored exact8 node against the reference's
SHAPES = {"64x96": LOGIT_SHAPES["64x96"], "512x512": (2, 512, 512)}
SITES_512 = ("x0_0", "x1_0", "x1_3a", "x3_1a")
INSIDE = (-6, -3, 3, 6)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def engines(torch_cuda):
    """one engine per (architecture, classes, shape, precision); every case loads its own state dict into it"""
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    cache = {}

    def get(arch, C, shape, precision):
        key = (arch, C, shape, precision)
        if key not in cache:
            B, H, W = shape
            if arch == "nested":
                m = NestedUNet(C, deep_supervision=True, precision=precision, max_batch=B, max_hw=(H, W))
            else:
                m = SimpleUNet(C, 3, precision=precision, max_batch=B, max_hw=(H, W))
            cache[key] = m.to("cuda:0").eval()
        return cache[key]
    yield get
    cache.clear()


def _read(model, name, shape):
    """unetpp_debug_read of any activation tensor of the engine (inner 'x1_0a', pooled 'x0_0p', single planes 'x1_0#hi')"""
    from unet_amd import _lib
    out = np.empty(shape, dtype=np.float32)
    n = _lib.load().unetpp_debug_read(model._handle, name.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
    assert n == out.size, (name, n, out.size, model._err(int(n)) if n < 0 else "")
    return out


def _shape_of(site, B, H, W, pooled=False):
    lvl = int(site[1])
    return (B, NB[lvl], H >> (lvl + pooled), W >> (lvl + pooled))


def _forward(torch, model, sd, xt):
    """load, clear the flags, one ordinary forward: (logits, mask, status)"""
    model.load_state_dict(sd, strict=True)
    model.debug_keep_intermediates(False)
    model.status(clear=True)
    mask, logits = model.segment(xt, return_logits=True)
    torch.cuda.synchronize()
    return logits.cpu().numpy(), mask.cpu().numpy(), model.status()


def _stored(torch, model, xt, names_shapes):
    """a second forward that keeps every tensor (x0_4 materialised, head unfused), then the named tensors read back"""
    model.debug_keep_intermediates(True)
    model(xt)
    torch.cuda.synchronize()
    out = {n: _read(model, n, s) for n, s in names_shapes}
    model.debug_keep_intermediates(False)
    return out


def _in_hbm(site, precision):
    return not (site == "x0_0a" and precision != "fast")      # the fused first block hands x0_0a over in LDS


def _sites(syn, shape_tag):
    return syn.NESTED_SITES if shape_tag == "64x96" else SITES_512


# ----------------------------------------------------------------------------- C.1
@pytest.mark.parametrize("shape_tag", list(SHAPES))
def test_inside_the_window(shape_tag, torch_cuda, engines, syn, oracle):
    torch = torch_cuda
    B, H, W = SHAPES[shape_tag]
    sd, x = nested_case(3, B, H, W)
    xt = torch.from_numpy(x).cuda()
    _, base = reference_tensors(oracle, sd, x)
    # x0_4 is never stored on the product path (the fused head reads fp32 registers), so its window is the whole sweep; only
    # the debug path that materialises it for a read-back splits it into planes, and that copy has the window of every other
    # stored tensor: it is read back from the highest window_low of the stored sites upwards
    stored_low = max(window_low(s) for s in syn.NESTED_SITES if s != "x0_4")
    readable = lambda site, prec, k: _in_hbm(site, prec) and (site != "x0_4" or k >= stored_low)
    failures = []
    print(f"\nC.1 {shape_tag}: site k peak | exact: dlogit node/peak status | exact8: dlogit flips node/peak status")
    for site in _sites(syn, shape_tag):
        top = k_hi(float(base[site].max()))
        for k in sorted({window_low(site), top} | {k for k in INSIDE if window_low(site) <= k <= top}):
            rs = syn.rescale_state_dict(sd, site, k)
            ref, t = reference_tensors(oracle, rs, x)
            ref_mask = oracle.masks_from_logits(ref)[0]
            margin = oracle.top2_margin(ref)
            peak = float(t[site].max())
            row = f"  {site:<6} {k:>3} {peak:9.3g} |"
            for prec, bar, node_bar in (("exact", EXACT_SMALL_BAR, EXACT_SMALL_BAR), ("exact8", NORTH_STAR, X8_NODE_BAR)):
                m = engines("nested", 3, SHAPES[shape_tag], prec)
                lg, mask, st = _forward(torch, m, rs, xt)
                err = float(np.abs(lg - ref).max())
                flips = mask != ref_mask
                rel = float("nan")
                if readable(site, prec, k):
                    got = _stored(torch, m, xt, [(site, _shape_of(site, B, H, W))])[site]
                    rel = float(np.abs(got - t[site]).max()) / peak
                row += f" {err:.2e} {int(flips.sum()):>3} {rel:.1e} {st} |"
                if not err < bar:
                    failures.append(f"{site} k={k} {prec}: logit error {err:.3e} above {bar}")
                if (flips & (margin > 2 * err + 1e-7)).any():
                    failures.append(f"{site} k={k} {prec}: a flipped mask pixel is not a near-tie")
                if readable(site, prec, k) and not rel < node_bar:
                    failures.append(f"{site} k={k} {prec}: stored tensor off by {rel:.2e} of its largest value (bar {node_bar})")
                if st != 0:
                    failures.append(f"{site} k={k} {prec}: status {st}")
            print(row)
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------- C.2
def test_below_the_window_the_device_loses_no_more_than_the_documented_arithmetic(torch_cuda, engines, syn, oracle):
    """Measured on the device (this table is also DESIGN.md §3 "Range"): see the printed rows.  The emulation is the prediction
    of DESIGN §3's arithmetic in float64, so a device error far BELOW it would mean the emulation is wrong about something;
    the ratio is printed for that reason."""
    import exact_emulation as em
    torch = torch_cuda
    B, H, W = SHAPES["64x96"]
    sd, x = nested_case(3, B, H, W)
    xt = torch.from_numpy(x).cuda()
    m = engines("nested", 3, (B, H, W), "exact")
    failures = []
    print("\nC.2 2x64x96 exact: site k peak | device dlogit | emulated dlogit | ratio | status")
    for site in syn.NESTED_SITES:
        for k in below_window(site):
            rs = syn.rescale_state_dict(sd, site, k)
            ref, t = reference_tensors(oracle, rs, x)
            emu = float(np.abs(em.exact_forward(rs, x) - ref).max())
            lg, _, st = _forward(torch, m, rs, xt)
            err = float(np.abs(lg - ref).max())
            peak = float(t[site].max())
            print(f"  {site:<6} {k:>3} {peak:9.3g} | {err:.2e} | {emu:.2e} | {err / emu:5.2f} | {st}")
            if not err <= 2 * emu + EXACT_SMALL_BAR:
                failures.append(f"{site} k={k}: device {err:.3e} > 2 x emulation {emu:.3e} + 2e-5")
            if st != 0:
                failures.append(f"{site} k={k}: status {st} (nothing left the fp16 range)")
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------- C.3
def _has_untouched_segment(a):
    """at least one run of 32 consecutive pixels of one row and channel (the whole row where it is shorter) entirely below
    65504, next to at least one element above: clamped and untouched tiles both occur"""
    seg = min(32, a.shape[3])
    rows = a[..., : a.shape[3] // seg * seg].reshape(a.shape[0], a.shape[1], a.shape[2], -1, seg)
    return bool((rows.max(axis=-1) < F16_MAX).any()) and float(a.max()) > F16_MAX


FAST_NODE_BAR = 5e-3                      # `fast` logits are off by 1.6e-3 ... 6.6e-3 at values around 1


def _c3_bounds(prec, peak):
    """(margin, tol) of clamp_check.  `exact`: 1e-4 and 2e-5 (its error, 2e-5 of the tensor's largest value, is below
    1e-4 x 65504 even when the tensor peaks 4x over the limit).  The other two modes compute the unclamped fp32 value less
    precisely -- to their node bar times the tensor's LARGEST value, which at k_hi + 2 is up to 3.6 x 65504 -- so an element the
    reference puts 1e-4 over the limit may legitimately come out just under it: margin and tolerance are that bar, scaled."""
    if prec == "exact":
        return 1e-4, EXACT_SMALL_BAR
    bar = (X8_NODE_BAR if prec == "exact8" else FAST_NODE_BAR) * max(1.0, peak / F16_MAX)
    return max(1e-4, bar), bar


PREC_C3 = ("exact", "exact8", "fast")


@pytest.mark.parametrize("shape_tag", list(SHAPES))
def test_over_the_top(shape_tag, torch_cuda, engines, syn, oracle):
    import torch.nn.functional as F
    torch = torch_cuda
    B, H, W = SHAPES[shape_tag]
    sd, x = nested_case(3, B, H, W)
    xt = torch.from_numpy(x).cuda()
    _, base = reference_tensors(oracle, sd, x)
    x8_top = float(torch.tensor(F16_MAX / 8).to(torch.float8_e5m2).float())
    failures = []
    print(f"\nC.3 {shape_tag}: site k | share of elements over 65504 | per precision: status, findings")
    for site in _sites(syn, shape_tag):
        if site == "x0_4":      # stays in fp32 registers in front of the fused head: never stored, so nothing to clamp or flag
            rs = syn.rescale_state_dict(sd, site, k_hi(float(base[site].max())) + 2)
            ref = oracle.torch_forward(rs, x)
            for prec, bar in (("exact", EXACT_SMALL_BAR), ("exact8", NORTH_STAR)):
                lg, _, st = _forward(torch, engines("nested", 3, SHAPES[shape_tag], prec), rs, xt)
                err = float(np.abs(lg - ref).max())
                print(f"  x0_4 (fused head, not stored) {prec}: max|dlogit| {err:.2e}, status {st}")
                if not (err < bar and st == 0):
                    failures.append(f"x0_4 {prec}: error {err:.3e}, status {st}")
            continue
        for k in (k_hi(float(base[site].max())) + 2, k_hi(float(base[site].max())) + 1):
            rs = syn.rescale_state_dict(sd, site, k)
            ref, t = reference_tensors(oracle, rs, x)
            if _has_untouched_segment(t[site]):
                break
        assert _has_untouched_segment(t[site]), f"{site}: no k with clamped and untouched segments"       # precondition
        over = t[site] > F16_MAX * (1 + 1e-4)
        row = f"  {site:<6} {k:>3} | {float(over.mean()):6.2%} |"
        for prec in PREC_C3:
            margin, tol = _c3_bounds(prec, float(t[site].max()))
            m = engines("nested", 3, SHAPES[shape_tag], prec)
            bad = []
            _, _, st = _forward(torch, m, rs, xt)
            if not st & OVERFLOW:
                bad.append("OVERFLOW not set")
            if st & NAN:
                bad.append("NAN set")
            if m.status() != st or m.status(clear=True) != st or m.status() != 0:
                bad.append("flag not sticky until cleared")
            pooled = site + "p" if site[3] == "0" and not site.endswith("a") and site != "x4_0" else None
            if _in_hbm(site, prec):
                names = [(site, _shape_of(site, B, H, W))]
                if pooled:
                    names.append((pooled, _shape_of(site, B, H, W, True)))
                if prec == "exact8":
                    names += [(site + "#lo", names[0][1]), (site + "#x8", names[0][1]), (site + "#hi", names[0][1])]
                got = _stored(torch, m, xt, names)
                for n, _ in names[:1 + bool(pooled)]:
                    why = clamp_check(got[n], t[n], margin, tol)
                    if why:
                        bad.append(f"{n}: {why}")
                if prec == "exact8":
                    over = t[site] > F16_MAX * (1 + margin)
                    if not (got[site + "#lo"][over] == 0).all():
                        bad.append("lo8 plane of a clamped element is not 0")
                    if not (got[site + "#x8"][over] == x8_top).all():
                        bad.append(f"x8 plane of a clamped element is not e5m2(65504 / 8) = {x8_top}")
                    if not (got[site + "#hi"][over] == F16_MAX).all():
                        bad.append("hi plane of a clamped element is not 65504")
            else:
                # x0_0a: conv0_0.conv2 in float64 on the clamped reference tensor is what x0_0 must be
                w = torch.from_numpy(rs["conv0_0.conv2.weight"]).double(); b = torch.from_numpy(rs["conv0_0.conv2.bias"]).double()
                s = torch.from_numpy(rs["conv0_0.bn2.weight"]).double() / torch.sqrt(torch.from_numpy(rs["conv0_0.bn2.running_var"]).double() + oracle.BN_EPS)
                y = F.conv2d(torch.from_numpy(np.minimum(t["x0_0a"], np.float32(F16_MAX))).double(), w, b, padding=1)
                y = torch.relu((y - torch.from_numpy(rs["conv0_0.bn2.running_mean"]).double()[None, :, None, None]) * s[None, :, None, None]
                               + torch.from_numpy(rs["conv0_0.bn2.bias"]).double()[None, :, None, None]).numpy()
                got = _stored(torch, m, xt, [("x0_0", _shape_of("x0_0", B, H, W))])["x0_0"]
                d = float(np.abs(got - y).max()) / float(y.max())
                if not d < (EXACT_SMALL_BAR if prec == "exact" else X8_NODE_BAR):
                    bad.append(f"x0_0 behind the clamped x0_0a off by {d:.2e} of its largest value")
            m.status(clear=True)
            _, _, st2 = _forward(torch, m, sd, xt)                # sticky, not stuck: an in-range forward leaves it clean
            if st2 != 0:
                bad.append(f"status {st2} after a clear and an in-range forward")
            row += f" {prec}: {st}" + (" " + "; ".join(bad) if bad else " ok") + " |"
            failures += [f"{site} k={k} {prec}: {b_}" for b_ in bad]
        print(row)
    assert not failures, "\n".join(failures)


def _simple_tensors(sd, x):
    """SimpleUNet.forward (simple_unet.py:94-128) through ATen's CPU ops, every tensor the engine stores by the engine's name"""
    import torch
    import torch.nn.functional as F
    T = lambda n: torch.from_numpy(sd[n])
    t = {}
    with torch.no_grad():
        def cr2(v, name, tn):
            t[tn + "a"] = F.relu(F.conv2d(v, T(f"{name}.0.weight"), T(f"{name}.0.bias"), padding=1))
            t[tn] = F.relu(F.conv2d(t[tn + "a"], T(f"{name}.2.weight"), T(f"{name}.2.bias"), padding=1))
            return t[tn]
        v = torch.from_numpy(x)
        for l in (1, 2, 3, 4):
            v = cr2(v if l == 1 else F.max_pool2d(v, 2, 2), f"enc{l}", f"enc{l}")
            if l < 4:
                t[f"enc{l}p"] = F.max_pool2d(v, 2, 2)
        for l in (3, 2, 1):
            t[f"up{l}t"] = F.conv_transpose2d(v, T(f"up{l}.weight"), T(f"up{l}.bias"), stride=2)
            v = cr2(torch.cat([t[f"up{l}t"], t[f"enc{l}"]], 1), f"dec{l}", f"dec{l}")
        logits = F.conv2d(v, T("final.weight"), T("final.bias"))
    return logits.numpy(), {n: a.numpy() for n, a in t.items()}


def test_over_the_top_simple_unet(torch_cuda, engines, syn, oracle):
    """SimpleUNet: one encoder conv with the fused pool (enc2), one transposed conv (up2t: its values are signed, so both ends
    of the range clamp) and one two-source decoder conv (dec2a), three precisions."""
    torch = torch_cuda
    shape = (2, 64, 96)
    B, H, W = shape
    sd = syn.make_simple_state_dict(7, 3, 0)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 7))
    xt = torch.from_numpy(x).cuda()
    ref0, base = _simple_tensors(sd, x)
    assert np.array_equal(ref0, oracle.simple_unet_torch_forward(sd, x))
    failures = []
    print("\nC.3 SimpleUNet 2x64x96: site k | per precision: status, findings")
    for site in ("enc2", "up2t", "dec2a"):
        k = k_hi(float(np.abs(base[site]).max())) + 2
        rs = syn.rescale_simple_state_dict(sd, site, k)
        ref, t = _simple_tensors(rs, x)
        assert np.array_equal(ref, ref0)
        assert _has_untouched_segment(np.abs(t[site]))
        lvl = int(site.rstrip("atp")[-1]) - 1
        shp = lambda extra=0: (B, (64, 128, 256, 512)[lvl], H >> (lvl + extra), W >> (lvl + extra))
        row = f"  {site:<6} {k:>3} |"
        for prec in PREC_C3:
            margin, tol = _c3_bounds(prec, float(np.abs(t[site]).max()))
            m = engines("simple", 7, shape, prec)
            bad = []
            _, _, st = _forward(torch, m, rs, xt)
            if not st & OVERFLOW or st & NAN:
                bad.append(f"status {st}")
            if m.status() != st or m.status(clear=True) != st or m.status() != 0:
                bad.append("flag not sticky until cleared")
            names = [(site, shp())] + ([(site + "p", shp(1))] if site == "enc2" else [])
            got = _stored(torch, m, xt, names)
            for n, _ in names:
                why = clamp_check(got[n], t[n], margin, tol)                        # up2t clamps at -65504 as well
                if why:
                    bad.append(f"{n}: {why}")
            m.status(clear=True)
            _, _, st2 = _forward(torch, m, sd, xt)
            if st2 != 0:
                bad.append(f"status {st2} after a clear and an in-range forward")
            row += f" {prec}: {st}" + (" " + "; ".join(bad) if bad else " ok") + " |"
            failures += [f"{site} k={k} {prec}: {b_}" for b_ in bad]
        print(row)
    assert not failures, "\n".join(failures)


def test_a_tensor_peaking_at_50000_raises_no_flag_simple_unet(torch_cuda, engines, syn, oracle):
    """The opposite of the overflow cases: SimpleUNet tensors at k_hi (peaks of 29,000 ... 59,000) raise no flag and meet
    parity relative to their size, in the two exact modes."""
    torch = torch_cuda
    shape = (2, 64, 96)
    B, H, W = shape
    sd = syn.make_simple_state_dict(7, 3, 0)
    x = syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, "smooth", 7))
    xt = torch.from_numpy(x).cuda()
    ref, base = _simple_tensors(sd, x)
    scale = max(1.0, float(np.abs(ref).max()))
    for site in ("enc2", "up2t", "dec2a"):
        k = k_hi(float(np.abs(base[site]).max()))
        rs = syn.rescale_simple_state_dict(sd, site, k)
        for prec, bar in (("exact", EXACT_SMALL_BAR), ("exact8", NORTH_STAR)):
            lg, _, st = _forward(torch, engines("simple", 7, shape, prec), rs, xt)
            err = float(np.abs(lg - ref).max()) / scale
            print(f"SimpleUNet {site} k={k} {prec}: max|dlogit| / max(1, max|logit|) = {err:.2e}, status {st}")
            assert err < bar and st == 0, (site, prec)


# ----------------------------------------------------------------------------- C.4
X8_LARGEST_OK = {}


@pytest.mark.parametrize("C,shape_tag,k", LOGIT_CASES)
def test_logit_scale(C, shape_tag, k, torch_cuda, engines, syn, oracle):
    """final.weight and final.bias x 2^k: logits up to +-70.  `exact` stays inside the absolute 1e-3; `exact8`'s error is relative
    to the logits, so its bar is twice its committed emulation's error on the same case, and the largest |logit| at which it
    still meets 1e-3 absolute on the device is recorded (printed by the last case; INTEGRATION.md carries it)."""
    import exact8_emulation as em8
    torch = torch_cuda
    shape = LOGIT_SHAPES[shape_tag]
    B, H, W = shape
    sd, x = nested_case(C, B, H, W)
    rs = syn.rescale_state_dict(sd, "logits", k)
    xt = torch.from_numpy(x).cuda()
    ref = oracle.torch_forward(rs, x)
    ref_mask = oracle.masks_from_logits(ref)[0]
    margin = oracle.top2_margin(ref)
    p64 = softmax64(ref)
    big = float(np.abs(ref).max())
    emu8 = float(np.abs(em8.exact8_forward(rs, x) - ref).max())
    for prec in ("exact", "exact8"):
        m = engines("nested", C, shape, prec)
        lg, mask, st = _forward(torch, m, rs, xt)
        err = float(np.abs(lg - ref).max())
        flips = mask != ref_mask
        probs = m.predict_proba(xt)
        torch.cuda.synchronize()
        probs = probs.cpu().numpy()
        perr = float(np.abs(probs - p64).max())
        rowsum = float(np.abs(probs.astype(np.float64).sum(axis=1) - 1.0).max())
        print(f"logits x 2^{k} C={C} {shape_tag} {prec}: largest |logit| {big:.1f}, max|dlogit| {err:.2e}"
              + (f" (emulated {emu8:.2e})" if prec == "exact8" else "") + f", flips {int(flips.sum())}, max|dprob| {perr:.2e}, "
              f"|row sum - 1| {rowsum:.1e}, status {st}")
        if prec == "exact":
            assert err < NORTH_STAR
        else:
            assert err <= 2 * emu8 + EXACT_SMALL_BAR
            if err < NORTH_STAR:
                X8_LARGEST_OK[(C, shape_tag)] = max(X8_LARGEST_OK.get((C, shape_tag), 0.0), big)
        assert not (flips & (margin > 2 * err + 1e-7)).any(), "a flipped mask pixel is not a near-tie"
        assert np.isfinite(lg).all() and np.isfinite(probs).all()
        assert perr <= 0.5 * err + 1e-6
        assert rowsum <= 8 * 2.0 ** -23
        assert st == 0
        for rule, params in RULES:
            cable, tape = m.segment_thresholded(xt, rule=rule, **params)
            torch.cuda.synchronize()
            rc, rt, _ = oracle.rule_masks_from_logits(ref, rule, **params)
            diff = (cable.cpu().numpy() != rc) | (tape.cpu().numpy() != rt)
            near = boundary_distance(p64, rule, params) <= 2 * perr
            print(f"    {rule}: {int(diff.sum())} pixels differ, {float(near.mean()):.3%} within 2 x {perr:.1e} of a boundary")
            assert not (diff & ~near).any(), rule
            assert float(near.mean()) <= 0.005, rule
    if (C, shape_tag, k) == LOGIT_CASES[-1]:
        print("largest |logit| at which exact8 met 1e-3 absolute on the device:", {f"C={c} {s}": round(v, 1) for (c, s), v in X8_LARGEST_OK.items()})
