"""The forward pass over the float32 input domain (device side; tests/test_input_domain_host.py is the CPU side and says why).

The six engine kinds -- NestedUNet and SimpleUNet, each in `exact`, `exact8` and `fast` -- cover the four pieces of code that ingest
the caller's tensor: the fused first block's patch loader (conv3x3_ws.h C0F patch_fetch / patch_store: NestedUNet `exact` and
`exact8`) and convert_input_kernel<1>, <2> and <2, true> (aux_kernels.h: NestedUNet `fast`, SimpleUNet in the three precisions).
Inputs are `synthetic.make_inputs_f32`'s families: k/255 as the control, ImageNet-normalised, raw bytes, +-255 with full
mantissas, normal, negated, 1e-3-sized, float32 subnormals, +-2^e over 37 octaves, impulses on the first block's tile seams,
zeros of both signs.  Shapes (test_input_domain_host.CASES): NestedUNet 2x32x48 under the device's own plan, NestedUNet 1x48x80
planned for two compute units (each workgroup walks several tiles: the patch double buffer and its prefetch carry signed
data), SimpleUNet 2x24x40.  Every case is one or two forwards of a tiny batch; oracle and emulations are cached per (case, kind).

  a  end to end against the oracle, s = max(1, max|reference logit|): `exact` 2e-5 s (SimpleUNet 5e-5 s); `exact8` twice the
     committed emulation's error on the same case + the exact bar, never above 1e-3 s (SimpleUNet: 1e-3 s); `fast` twice its
     emulation's error + the exact bar, never above 5e-2 s; mask flips only at near-ties of the reference; status 0; finite.
  b  the ingest step by itself: `in8` and its planes bit for bit (signs of zero included) against the host's split; x0_0 /
     x0_0a / enc1a against the first layer computed on the host.
  c  identities, bitwise: signed zeros, uint8 frames against their k/255 tensor, non-contiguous forms; refused dtypes / shapes.
(d, the range flags on inputs at and beyond +-65504, is tests/test_range_status.py.)

Run on the GPU box:  python -m pytest tests -m gpu"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_fast import MAX_SHARE, Reader
from test_gpu_plan_sweep import family, plan_env, run_with_plan
from test_gpu_value_range import X8_NODE_BAR
from test_input_domain_host import (CASES, EXACT_BAR, PRECISIONS, SEED, bits_equal, device_cap, emulated_error, first_block64,
                                    inputs, reference, scale_of, simple_enc1a64, state_dict)

sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

ENGINE_CASES = [(case, prec) for case in CASES for prec in PRECISIONS]
ARCH_PREC = [(arch, prec) for arch in ("nested", "simple") for prec in PRECISIONS]
IDENTITY_SHAPE = (2, 32, 48)
# exact8, the first block on x: mean |device - fp32 arithmetic| over mean |device - emulation| that
# exact8_emulation.layer_agreement must show (tests/test_gpu_exact8.py asserts 10 on `unit`, measured 22)
X8_FIRST_BLOCK_RATIO = 10.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def engines(torch_cuda):
    """one engine per (architecture, classes, shape, precision, plan switches), created under its switches (the first forward
    creates it; the switches are gone again afterwards) with `sd` loaded"""
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    cache = {}

    def get(arch, C, shape, precision, sd, switches=()):
        key = (arch, C, shape, precision, tuple(sorted(dict(switches).items())))
        if key not in cache:
            B, H, W = shape
            if arch == "nested":
                m = NestedUNet(C, deep_supervision=True, precision=precision, max_batch=B, max_hw=(H, W))
            else:
                m = SimpleUNet(C, 3, precision=precision, max_batch=B, max_hw=(H, W))
            m = m.to("cuda:0").eval()
            m.load_state_dict(sd, strict=True)
            with plan_env(**dict(switches)):
                m(torch.zeros((B, 3, H, W), dtype=torch.float32, device="cuda:0"))
            torch.cuda.synchronize()
            assert m.status() == 0
            cache[key] = m
        return cache[key]
    yield get
    cache.clear()


def case_engine(engines, case, prec):
    arch, C, shape, _, switches = CASES[case]
    return engines(arch, C, shape, prec, state_dict(case), switches)


def signed_equal(a, b):
    """float64 tensors equal element by element, the sign of a zero included"""
    import torch
    return a.shape == b.shape and torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


def host_planes(prec, x):
    """{debug-read name: float64 tensor [B, 8, H, W]} of `in8` as the host splits x (channels 3..7 are +0.0)"""
    import torch
    import exact8_emulation as em8
    import exact_emulation as em
    import fast_emulation as fe
    if prec == "fast":
        return {"in8": fe.input_plane(x)}
    x8 = torch.cat([fe._t(x), torch.zeros(x.shape[0], 5, *x.shape[2:], dtype=torch.float64)], 1)
    if prec == "exact":
        a = em.Act(x8)
        return {"in8#hi": a.h, "in8#lo": a.l, "in8": fe._f32(a.value)}
    a = em8.Act(x8)
    return {"in8#hi": a.h, "in8#lo": a.l8, "in8#x8": a.x8, "in8": fe._f32(a.value)}


# ----------------------------------------------------------------------------- a. end to end
@pytest.mark.parametrize("case,prec", ENGINE_CASES)
def test_end_to_end_against_the_oracle(case, prec, torch_cuda, engines, syn, oracle):
    torch = torch_cuda
    m = case_engine(engines, case, prec)
    failures = []
    print(f"\na. {case} {prec}: kind | max|logit| | max|dlogit| / s | cap / s | emulated / s | flips | status")
    for kind in syn.PARITY_INPUT_KINDS:
        ref = reference(case, kind)[0]
        ref_mask = oracle.masks_from_logits(ref)[0]
        s = scale_of(ref)
        cap = device_cap(case, kind, prec)
        emu = emulated_error(case, kind, prec)
        m.status(clear=True)
        mask, logits = m.segment(torch.from_numpy(inputs(case, kind)).cuda(), return_logits=True)
        torch.cuda.synchronize()
        st = m.status()
        lg, mk = logits.cpu().numpy(), mask.cpu().numpy()
        err = float(np.abs(lg - ref).max())
        flips = mk != ref_mask
        print(f"  {kind:<9} {float(np.abs(ref).max()):9.4g} | {err / s:.2e} | {cap / s:.2e} | "
              + ("-" if emu is None else f"{emu / s:.2e}") + f" | {int(flips.sum()):>3} | {st}")
        if not np.isfinite(lg).all():
            failures.append(f"{kind}: a logit is not finite")
        if not err <= cap:
            failures.append(f"{kind}: max|dlogit| {err:.3e} above {cap:.3e} ({err / s:.2e} of s against {cap / s:.2e})")
        if (flips & (oracle.top2_margin(ref) > 2 * err + 1e-7)).any():
            failures.append(f"{kind}: a flipped mask pixel is not a near-tie")
        if st != 0:
            failures.append(f"{kind}: status {st} (no tensor of the reference reaches 2^15)")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("prec", ["exact", "exact8"])
def test_the_planned_first_block_walks_several_tiles(prec, torch_cuda, engines):
    """what nested-1x48x80 is for: planned for two compute units, each workgroup of the fused first block fetches the next
    tile's patch of signed samples while it computes the current one"""
    torch = torch_cuda
    case = "nested-1x48x80"
    m = case_engine(engines, case, prec)
    x = torch.from_numpy(inputs(case, "imagenet")).cuda()
    _, plan = run_with_plan(torch, m, lambda: m(x))
    first = [p for p in plan if family(p[0]) == "first block"]
    assert len(first) == 1, [p[0] for p in plan]
    _, grid, tiles, _, _ = first[0]
    print(f"{case} {prec}: the first block runs {tiles} tiles on {grid} workgroups")
    assert 1 <= grid <= 2 and tiles >= 2 * grid


# ----------------------------------------------------------------------------- b. the ingest step by itself
@pytest.mark.parametrize("case,prec", ENGINE_CASES)
def test_ingest_step(case, prec, torch_cuda, engines, syn):
    """`in8` where the engine materialises it (NestedUNet `fast`, SimpleUNet): the host's split, bit for bit, for all thirteen
    kinds.  Then the first layer: NestedUNet `exact` / `exact8` x0_0 against the float64 first block on x (the fused first
    block leaves nothing earlier in memory), `fast` x0_0a and SimpleUNet enc1a from the device's own `in8`."""
    import exact8_emulation as em8
    import fast_emulation as fe
    torch = torch_cuda
    arch, _, (B, H, W), _, _ = CASES[case]
    sd = state_dict(case)
    m = case_engine(engines, case, prec)
    has_in8 = arch == "simple" or prec == "fast"
    failures = []
    print(f"\nb. {case} {prec}: kind | first layer")
    m.debug_keep_intermediates(True)
    try:
        for kind in syn.INPUT_KINDS:
            x = inputs(case, kind)
            m.status(clear=True)
            m(torch.from_numpy(x).cuda())
            torch.cuda.synchronize()
            rd = Reader(m, B, H, W, fe)
            if m.status() != 0:
                failures.append(f"{kind}: status {m.status()}")
            if has_in8:
                for name, want in host_planes(prec, x).items():
                    if not signed_equal(rd(name), want):
                        bad = (rd(name) != want) | (torch.signbit(rd(name)) != torch.signbit(want))
                        failures.append(f"{kind}: {name} differs from the host's split in {int(bad.sum())} elements")
            if arch == "nested" and prec != "fast":
                got = rd.np("x0_0")
                ref = first_block64(sd, x)
                if prec == "exact":
                    rel = float(np.abs(got - ref).max()) / scale_of(ref)
                    row = f"x0_0 within {rel:.2e} of max(1, its largest value)"
                    if not rel <= EXACT_BAR["nested"]:
                        failures.append(f"{kind}: {row}")
                else:
                    d_emu, d_ref, differ = em8.layer_agreement(got, em8.first_block(x, sd), fe._t(ref))
                    row = (f"x0_0 mean|device - emulation| {d_emu:.2e}, mean|device - fp32 arithmetic| {d_ref:.2e} "
                           f"(ratio {d_ref / max(d_emu, 1e-300):.1f}), {differ:.2%} of the elements differ")
                    if not (d_emu * X8_FIRST_BLOCK_RATIO < d_ref and differ < 0.12):
                        failures.append(f"{kind}: {row}")
            elif prec == "fast":
                name, wb = ("x0_0a", fe._fold(sd, "conv0_0.conv1")) if arch == "nested" else ("enc1a", fe._plain(sd, "enc1.0"))
                used, share = fe.layer_check(rd.np(name), *fe.conv(rd("in8"), *wb), fe.GAMMA["conv"])
                row = f"{name} uses {used:.3f} of 4 gamma S, {share:.4%} of the elements differ from the emulation"
                if not (used <= 1.0 and share <= MAX_SHARE):
                    failures.append(f"{kind}: {row}")
            else:
                got = rd.np("enc1a")
                ref = simple_enc1a64(sd, x)
                bar = EXACT_BAR["simple"] if prec == "exact" else X8_NODE_BAR
                rel = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
                row = f"enc1a within {rel:.2e} of its largest value (bar {bar})"
                if not rel <= bar:
                    failures.append(f"{kind}: {row}")
            print(f"  {kind:<12} {row}")
    finally:
        m.debug_keep_intermediates(False)
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------- c. identities
def _identity_engine(engines, syn, arch, prec):
    sd = syn.make_state_dict(3, 3, True, 2) if arch == "nested" else syn.make_simple_state_dict(7, 3, 0)
    return engines(arch, 3 if arch == "nested" else 7, IDENTITY_SHAPE, prec, sd)


def _outputs(torch, m, x):
    mask, logits = m.segment(x, return_logits=True)
    torch.cuda.synchronize()
    return logits.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("arch,prec", ARCH_PREC)
def test_identities_bitwise(arch, prec, torch_cuda, engines, syn):
    torch = torch_cuda
    B, H, W = IDENTITY_SHAPE
    m = _identity_engine(engines, syn, arch, prec)
    same = lambda a, b: bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    out = lambda x: _outputs(torch, m, x)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # -0.0 is 0: the sign of a zero sample must not reach a logit
    assert same(out(dev(syn.make_inputs_f32("signed_zeros", B, H, W, SEED))), out(dev(syn.make_inputs_f32("zeros", B, H, W, SEED))))
    # a uint8 frame and its k/255 tensor
    frames = syn.make_frames_u8(B, H, W, "smooth", SEED)
    assert same(out(dev(frames)), out(dev(syn.frames_to_chw_f32(frames))))
    # forms of one tensor: each gives the bits of its .contiguous() copy
    big = syn.make_inputs_f32("imagenet", 4, 64, 80, SEED)
    forms = {
        "channels_last": dev(big[:2, :, :H, :W]).contiguous(memory_format=torch.channels_last),
        "batch slice": dev(big)[1:3, :, :H, :W],
        "crop view": dev(big[:2])[:, :, 16:48, 16:64],
        "expanded frame": dev(big[:1, :, :H, :W]).expand(B, 3, H, W),
    }
    for tag, v in forms.items():
        assert tuple(v.shape) == (B, 3, H, W), tag
        if tag != "batch slice":
            assert not v.is_contiguous(), tag
        assert same(out(v), out(v.contiguous().clone())), tag
    assert m.status() == 0


@pytest.mark.parametrize("arch,prec", ARCH_PREC)
def test_refused_inputs(arch, prec, torch_cuda, engines, syn):
    torch = torch_cuda
    B, H, W = IDENTITY_SHAPE
    m = _identity_engine(engines, syn, arch, prec)
    x = torch.from_numpy(syn.make_inputs_f32("unit", B, H, W, SEED)).cuda()
    for dtype in (torch.float16, torch.bfloat16, torch.float64, torch.int8):
        with pytest.raises(RuntimeError):
            m(x.to(dtype))
    for shape in ((B, 1, H, W), (B, 4, H, W)):
        with pytest.raises(RuntimeError):
            m(torch.zeros(shape, dtype=torch.float32, device="cuda:0"))
    with pytest.raises(RuntimeError):
        m(torch.zeros((B, H, W, 4), dtype=torch.uint8, device="cuda:0"))
    ref = _outputs(torch, m, x)                      # the refusals leave the engine as it was
    assert bits_equal(ref[0], _outputs(torch, m, x)[0]) and m.status() == 0
