"""Deep-supervision outputs [out, out1, out2, out3] and pruned UNet++ inference on the device, against the reference's own
deep-supervision forward (tests/golden/ds_*.npz, scripts/make_golden_ds.py) and the oracle.
Run on the GPU box:  python -m pytest tests -m gpu"""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

EXACT_TOL = 5e-5     # exact: fp32-class
LOGIT_TOL = 1e-3     # the project's gate (exact8)
DS = ((1, "ds1_3", "x1_3"), (2, "ds2_2", "x2_2"), (3, "ds3_1", "x3_1"))
PRUNED_AWAY = {1: ("conv0_4",), 2: ("conv1_3", "conv0_4"), 3: ("conv2_2", "conv1_3", "conv0_4")}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


def make_model(C, wseed, precision, syn, max_batch, hw, micro_batch=0, streams=1):
    from unet_amd.nested_unet import NestedUNet
    sd = syn.make_state_dict(C, 3, True, wseed)
    m = NestedUNet(C, deep_supervision=True, precision=precision, max_batch=max_batch, max_hw=hw,
                   micro_batch=micro_batch, streams=streams).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    return m.eval(), sd


def unexplained_flips(mask, ref_mask, ref_margin, err):
    return int(((mask != ref_mask) & (ref_margin >= 2 * err + 1e-7)).sum())


def oracle_ds(oracle, sd, x_np, H, W):
    """[out, out1, out2, out3] from the oracle's CPU graph: node -> F.conv2d (1x1) -> F.interpolate(size=(H, W))."""
    import torch
    import torch.nn.functional as F
    logits, t = oracle.torch_forward(sd, x_np, return_intermediates=True)
    outs = [logits]
    for k, head, node in DS:
        low = F.conv2d(torch.from_numpy(t[node]), torch.from_numpy(sd[head + ".weight"]), torch.from_numpy(sd[head + ".bias"]))
        outs.append(F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).numpy())
    return outs


@pytest.mark.parametrize("precision", ["exact", "exact8"])
@pytest.mark.parametrize("tag", ["ds_c3_64x64", "ds_c7_48x80"])
def test_against_reference_fixtures(tag, precision, torch_cuda, syn, oracle):
    torch = torch_cuda
    g = load_golden(tag)
    C, B, H, W = int(g["num_classes"]), int(g["B"]), int(g["H"]), int(g["W"])
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    assert hashlib.sha256(frames.tobytes()).hexdigest() == str(g["frames_sha"])
    model, _ = make_model(C, int(g["wseed"]), precision, syn, B, (H, W))
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    outs = model.forward_deep_supervision(x)
    masks = [model.segment(x, output=k) for k in range(4)]
    torch.cuda.synchronize()
    tol = EXACT_TOL if precision == "exact" else LOGIT_TOL
    errs = []
    for k in range(4):
        err = float(np.abs(outs[k].cpu().numpy() - g[f"out{k}"]).max())
        flips = unexplained_flips(masks[k].cpu().numpy(), g[f"mask{k}"], g[f"margin{k}"], err)
        print(f"{tag} {precision} out{k}: max|dlogit|={err:.3e} unexplained mask flips={flips}")
        errs.append((k, err, flips))
    over = [(k, err) for k, err, _ in errs if err > tol]
    assert not over, f"{precision}: outputs over the {tol:g} bar (k, max|dlogit|): {over}"
    assert all(f == 0 for _, _, f in errs), errs


def test_fast_mode_within_its_band(torch_cuda, syn):
    """fast (plain fp16) does not pass the 1e-3 gate; every output stays within its documented band (test_gpu_parity.py)."""
    torch = torch_cuda
    g = load_golden("ds_c3_64x64")
    C, B, H, W = int(g["num_classes"]), int(g["B"]), int(g["H"]), int(g["W"])
    model, _ = make_model(C, int(g["wseed"]), "fast", syn, B, (H, W))
    x = torch.from_numpy(syn.frames_to_chw_f32(syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"])))).cuda()
    outs = model.forward_deep_supervision(x)
    torch.cuda.synchronize()
    for k in range(4):
        err = float(np.abs(outs[k].cpu().numpy() - g[f"out{k}"]).max())
        print(f"fast out{k}: max|dlogit|={err:.3e}")
        assert 1e-6 < err < 3e-2, (k, err)


def _head_as_the_kernel(node, w, b):
    """head_generic_kernel's arithmetic on one frame: per class, s = bias, then s = fmaf(x[ch], w[ch], s) for ch = 0 .. Cx-1
    in order (the product is exact in float64, the sum rounds to float32)."""
    C, Cx = w.shape[0], w.shape[1]
    s = np.repeat(b.astype(np.float32)[:, None, None], node.shape[1] * node.shape[2], axis=1).reshape(C, *node.shape[1:])
    for ch in range(Cx):
        s = (node[ch][None].astype(np.float64) * w[:, ch, None, None].astype(np.float64) + s).astype(np.float32)
    return s


def test_upsample_kernel_pinned_apart_from_the_trunk(torch_cuda, syn):
    """ds head + ds_upsample_kernel alone, at extents where the index rule matters most (1024 and 2048: a contracted
    l1 = round(s * dst - i0) differs from ATen's round(round(s * dst) - i0) by up to 3e-5 there): the node x_k is read back
    from the engine, the head is restated as the kernel computes it, F.interpolate does the rest on the CPU -- and
    forward(x, output=k) must match within 1e-6 (a few ulp of the logits), free of the trunk's own error."""
    import torch.nn.functional as F
    torch = torch_cuda
    H, W = 1024, 2048
    frames = syn.make_frames_u8(1, H, W, "uniform", 31)
    model, sd = make_model(3, 4, "exact", syn, 1, (H, W))
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    for k, head, node in DS:
        got = model.forward(x, output=k)
        torch.cuda.synchronize()
        xk = model.debug_activation(node, 1, H, W)[0]              # the node this pruned pass just computed
        low = _head_as_the_kernel(xk, sd[head + ".weight"][:, :, 0, 0], sd[head + ".bias"])
        ref = F.interpolate(torch.from_numpy(low)[None], size=(H, W), mode="bilinear", align_corners=True)[0].numpy()
        err = float(np.abs(got[0].cpu().numpy() - ref).max())
        print(f"{H}x{W} out{k}: kernel vs CPU restatement on the read-back node: max|dlogit|={err:.3e}")
        assert err <= 1e-6, (k, err)


def test_config2_shape_microbatch_streams_and_tail(torch_cuda, syn, oracle):
    """3-class 512x512, B = 16 in passes of 4 on two internal streams; frames 0 and 15 against the oracle.  Then a
    batch of 6 (a tail pass of 2) on the same engine, frames 0 and 5."""
    torch = torch_cuda
    H = W = 512
    frames = np.stack([syn.make_frame_u8(H, W, i, ("smooth", "uniform")[i % 2], 1234) for i in range(16)])
    model, sd = make_model(3, 2, "exact", syn, 16, (H, W), micro_batch=4, streams=2)
    xf = syn.frames_to_chw_f32(frames)
    pick = [0, 5, 15]
    refs = oracle_ds(oracle, sd, xf[pick], H, W)
    x = torch.from_numpy(xf).cuda()
    for batch, frames_checked in ((16, (0, 15)), (6, (0, 5))):
        outs = model.forward_deep_supervision(x[:batch])
        masks = [model.segment(x[:batch], output=k) for k in range(4)]
        torch.cuda.synchronize()
        for k in range(4):
            for f in frames_checked:
                ref = refs[k][pick.index(f)]
                got = outs[k][f].cpu().numpy()
                err = float(np.abs(got - ref).max())
                srt = np.sort(ref, axis=0)
                flips = unexplained_flips(masks[k][f].cpu().numpy(), np.argmax(ref, axis=0), srt[-1] - srt[-2], err)
                print(f"B={batch} frame {f} out{k}: max|dlogit|={err:.3e} unexplained flips={flips}")
                assert err <= EXACT_TOL and flips == 0, (batch, f, k, err, flips)


@pytest.mark.parametrize("precision", ["exact", "exact8", "fast"])
def test_pruned_equals_full_bitwise(precision, torch_cuda, syn):
    torch = torch_cuda
    frames = syn.make_frames_u8(3, 64, 96, "smooth", 21)
    model, _ = make_model(3, 5, precision, syn, 3, (64, 96), micro_batch=2, streams=1)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    full = model.forward_deep_supervision(x)
    main = model(x)
    pruned = {k: model.forward(x, output=k) for k in (1, 2, 3)}
    m2, _ = make_model(3, 5, precision, syn, 3, (64, 96), micro_batch=2, streams=2)
    full2 = m2.forward_deep_supervision(x)
    torch.cuda.synchronize()
    assert torch.equal(full[0], main)
    for k in (1, 2, 3):
        assert torch.equal(pruned[k], full[k]), k
    for k in range(4):
        assert torch.equal(full2[k], full[k]), k
    assert all(bool(torch.isfinite(t).all()) for t in full)


def test_outputs_of_a_pruned_call(torch_cuda, syn, oracle):
    from test_oracle_golden import RULE_CASES
    torch = torch_cuda
    frames = syn.make_frames_u8(2, 64, 64, "uniform", 12)
    model, _ = make_model(3, 8, "exact", syn, 2, (64, 64))
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    for k in (1, 2, 3):
        logits = model.forward(x, output=k).cpu().numpy()
        mask, cable, tape = model.segment(x, return_class_masks=True, output=k)
        probs = model.predict_proba(x, output=k)
        torch.cuda.synchronize()
        mask = mask.cpu().numpy()
        assert np.array_equal(mask, np.argmax(logits, axis=1).astype(np.uint8)), k
        assert np.array_equal(cable.cpu().numpy(), (mask == 1).astype(np.uint8))
        assert np.array_equal(tape.cpu().numpy(), (mask == 2).astype(np.uint8))
        perr = float((probs.cpu() - torch.softmax(torch.from_numpy(logits), dim=1)).abs().max())
        assert perr < 1e-6, (k, perr)
        for key, rule, params in RULE_CASES:
            c, t, p = model.segment_thresholded(x, rule=rule, return_probs=True, output=k, **params)
            torch.cuda.synchronize()
            rc, rt = oracle.RULES[rule](np.transpose(p.cpu().numpy(), (0, 2, 3, 1)), **params)
            assert np.array_equal(c.cpu().numpy(), rc) and np.array_equal(t.cpu().numpy(), rt), (k, key)


def test_u8_bgr_input_equals_f32_input(torch_cuda, syn):
    torch = torch_cuda
    frames = syn.make_frames_u8(2, 48, 64, "uniform", 3)
    model, _ = make_model(3, 2, "exact", syn, 2, (48, 64))
    xf = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    xu = torch.from_numpy(frames).cuda()
    for k in (1, 2, 3):
        a = model.forward(xf, output=k)
        b = model.forward(xu, output=k)
        torch.cuda.synchronize()
        assert torch.equal(a, b), k


def test_pruning_really_prunes(torch_cuda, syn):
    torch = torch_cuda
    frames = syn.make_frames_u8(1, 64, 64, "smooth", 5)
    model, _ = make_model(3, 2, "exact", syn, 1, (64, 64))
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    model(x)
    torch.cuda.synchronize()

    def launches(fn):
        model.profile(True)
        fn()
        names = [r[0] for r in model.profile_read()]
        model.profile(False)
        return names

    main = launches(lambda: model(x))
    assert not [n for n in main if n.startswith("ds")]
    for k, head, _ in DS:
        names = launches(lambda: model.forward(x, output=k))
        print(f"output {k}: {len(names)} launches (full: {len(main)})")
        for lvl in PRUNED_AWAY[k]:
            assert not [n for n in names if lvl in n], (k, lvl, names)
        assert not [n for n in names if "final" in n]
        heads = [n for n in names if "|head_generic_kernel" in n]
        ups = [n for n in names if "|ds_upsample_kernel" in n]
        assert heads == [f"{head}|head_generic_kernel<2>"] and ups == [f"{head}+up|ds_upsample_kernel"], names
        assert names[-2:] == heads + ups            # the pass ends with this output's two launches ...
        assert names[:-2] == main[:len(names) - 2]  # ... after the full forward's launches up to the node's conv2
        assert main[len(names) - 2].startswith(("conv2_2", "conv1_3", "conv0_4")[3 - k])   # the first level it skips
    allds = launches(lambda: model.forward_deep_supervision(x))
    assert sum("|ds_upsample_kernel" in n for n in allds) == 3 and sum(n.startswith("ds") and "|head_generic" in n for n in allds) == 3
    assert [n for n in allds if not n.startswith("ds")] == main


def test_errors(torch_cuda, syn):
    torch = torch_cuda
    from unet_amd import _lib, packing
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    lib = _lib.load()
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    m0 = NestedUNet(3, deep_supervision=False, max_batch=1, max_hw=(32, 32)).to("cuda:0")
    m0.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    with pytest.raises(ValueError, match="deep_supervision=False"):
        m0.forward(x, output=1)
    s = SimpleUNet(7, max_batch=1, max_hw=(32, 32)).to("cuda:0")
    s.load_state_dict(syn.make_simple_state_dict(7, 3, 0), strict=True)
    s(x)
    with pytest.raises(NotImplementedError):
        s.segment(x, output=1)

    sd = syn.make_state_dict(3, 3, True, 2)
    m = NestedUNet(3, deep_supervision=True, max_batch=1, max_hw=(32, 32)).to("cuda:0")
    m.load_state_dict(sd, strict=True)
    m(x)                                             # engine exists, ds heads not uploaded yet
    torch.cuda.synchronize()
    y = torch.empty(1, 3, 32, 32, device="cuda")
    rec = _lib.Outputs(ctypes.c_void_p(y.data_ptr()), None, None, None, None, 0, 0.0, 0.0, 0.0, 0.0)
    P = ctypes.POINTER(_lib.Outputs)
    one = (P * 4)(None, ctypes.pointer(rec), None, None)
    none = (P * 4)()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp = ctypes.c_void_p(x.data_ptr())
    assert lib.unetpp_forward_ds(m._handle, xp, 0, 1, 32, 32, one, stream) == -4
    assert lib.unetpp_forward_ds(m._handle, xp, 0, 1, 32, 32, none, stream) == -1
    assert lib.unetpp_forward_ds(s._handle, xp, 0, 1, 32, 32, one, stream) == -2
    blob = packing.build_ds_blob(sd, 3)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.unetpp_load_ds_heads(m._handle, vp(blob), blob.nbytes - 4) == -1
    wrong = blob.copy(); wrong[:4] = np.frombuffer(b"UNPP", np.uint8)
    assert lib.unetpp_load_ds_heads(m._handle, vp(wrong), wrong.nbytes) == -1
    other = packing.build_ds_blob(syn.make_state_dict(7, 3, True, 2), 7)
    assert lib.unetpp_load_ds_heads(m._handle, vp(other), other.nbytes) == -1
    assert lib.unetpp_load_ds_heads(s._handle, vp(blob), blob.nbytes) == -2
    assert lib.unetpp_forward_ds(m._handle, xp, 0, 1, 32, 32, one, stream) == -4      # still nothing loaded
    m.status(clear=True)
    nan = blob.copy(); nan[32:].view(np.float32)[5] = np.nan
    assert lib.unetpp_load_ds_heads(m._handle, vp(nan), nan.nbytes) == 0
    assert m.status(clear=True) & _lib.STATUS_NAN
    assert lib.unetpp_load_ds_heads(m._handle, vp(blob), blob.nbytes) == 0
    assert m.status(clear=True) == 0
    assert lib.unetpp_forward_ds(m._handle, xp, 0, 1, 32, 32, one, stream) == 0
    torch.cuda.synchronize()
    # ds_upsample_kernel stores 4 pixels at once: misaligned buffers of outs[1..3] are refused
    z = torch.empty(1 * 3 * 32 * 32 + 4, device="cuda")
    for field, off in (("dev_logits", 4), ("dev_probs", 8), ("dev_mask", 1), ("dev_cable", 2), ("dev_tape", 3)):
        bad = _lib.Outputs(None, None, None, None, None, 0, 0.0, 0.0, 0.0, 0.0)
        setattr(bad, field, z.data_ptr() + off)
        assert lib.unetpp_forward_ds(m._handle, xp, 0, 1, 32, 32, (P * 4)(None, None, ctypes.pointer(bad), None), stream) == -1, field
    # new main weights drop the heads of the previous checkpoint (C callers included)
    main_blob = packing.build_blob(sd, 3)
    assert lib.unetpp_load_weights(m._handle, vp(main_blob), main_blob.nbytes) == 0
    assert lib.unetpp_forward_ds(m._handle, xp, 0, 1, 32, 32, one, stream) == -4
    assert lib.unetpp_load_ds_heads(m._handle, vp(blob), blob.nbytes) == 0
    m._ds_uploaded = False                           # the wrapper's view of the engine: re-uploaded on its next ds call
    assert torch.equal(m.forward(x, output=1), y)    # same checkpoint, same result as the raw call above
    # weights from a broadcast blob carry no ds heads: refused, not served from the heads the engine still holds
    m.load_weights_from_device_blob(torch.from_numpy(packing.build_blob(sd, 3)).cuda())
    with pytest.raises(RuntimeError, match="no deep-supervision heads"):
        m.forward(x, output=1)
    assert m.forward(x).shape == (1, 3, 32, 32)
