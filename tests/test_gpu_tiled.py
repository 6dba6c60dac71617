"""Sliding-window inference on the device (unetpp_tile_gather_u8, unetpp_tile_gate_f32, unetpp_tile_blend_f32 and the
NestedUNet methods built on them) against the NumPy restatement (unet_amd/tiling.py) and the fixtures made from the
reference's own predict methods (tests/golden/tiled_scenes.npz).  Gather, gate and blend are integer arithmetic, an
order-free maximum and float32 operations in a fixed order: exact equality of the bits.  Only the end-to-end test, which
runs the engine's network, has a tolerance: the project's 1e-3 logit bar.
Run on the GPU box:  python -m pytest tests/test_gpu_tiled.py -m gpu"""
import ctypes

import numpy as np
import pytest

from test_tiled_host import CASES, G, TAGS, bits, frame_rgb, sha
from unet_amd import tiling as tl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, deep_supervision=False, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: the parts need none


@pytest.fixture(scope="module")
def trained(torch_cuda, syn):
    """One engine per class count with the fixtures' weights; max_batch=4 so that the patch batches go in several chunks
    (12 = 4 + 4 + 4, 6 = 4 + 2)."""
    from unet_amd.nested_unet import NestedUNet
    out = {}
    for C in (2, 3):
        m = NestedUNet(C, deep_supervision=False, precision="exact", max_batch=4, max_hw=(64, 64)).to("cuda:0")
        m.load_state_dict(syn.make_trained_like_state_dict(C, 3, False, 0), strict=True)
        out[C] = m.eval()
    return out


def stored_include(c):
    return None if c["thr"] is None else (G[c["tag"] + "_scores"] >= np.float32(c["thr"]))


# ---- 1. the blend on the reference's own per-patch maps ------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_blend_equals_reference_bits(torch_cuda, model, tag):
    torch = torch_cuda
    c = CASES[TAGS.index(tag)]
    maps = torch.from_numpy(G[tag + "_maps"]).cuda()
    inc = stored_include(c)
    include = None if inc is None else torch.from_numpy(inc.astype(np.uint8)).cuda()
    mask, output = model.blend_tiles(maps, (c["H"], c["W"]), c["patch"], c["stride"], include=include)
    assert output.dtype == torch.float32 and tuple(output.shape) == (1, c["H"], c["W"], c["C"])
    assert np.array_equal(bits(output[0].cpu().numpy()), bits(G[tag + "_output"])), tag
    assert mask.dtype == torch.uint8 and np.array_equal(mask[0].cpu().numpy(), G[tag + "_mask"]), tag
    mask2, none = model.blend_tiles(maps, (c["H"], c["W"]), c["patch"], c["stride"], include=include, return_output=False)
    assert none is None and torch.equal(mask2, mask)


def test_blend_batch_of_two_frames_and_streams(torch_cuda, model):
    """Two frames of one shape in one launch (the ungated and the gated 48 x 150 case: the second frame drops a patch),
    twice, and once more on a second stream: each frame its own result, every time the same bits."""
    torch = torch_cuda
    a, b = CASES[TAGS.index("c2_48x150_probs")], CASES[TAGS.index("c2_48x150_gated")]
    maps = torch.from_numpy(np.concatenate([G[a["tag"] + "_maps"], G[b["tag"] + "_maps"]])).cuda()
    inc = np.concatenate([np.ones(4, bool), stored_include(b)]).astype(np.uint8)
    include = torch.from_numpy(inc).cuda()
    mask, output = model.blend_tiles(maps, (48, 150), 64, 32, include=include)
    for i, c in enumerate((a, b)):
        assert np.array_equal(bits(output[i].cpu().numpy()), bits(G[c["tag"] + "_output"])), c["tag"]
        assert np.array_equal(mask[i].cpu().numpy(), G[c["tag"] + "_mask"]), c["tag"]
    mask2, output2 = model.blend_tiles(maps, (48, 150), 64, 32, include=include)
    assert torch.equal(mask2, mask) and torch.equal(output2.view(torch.int32), output.view(torch.int32))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        mask3, output3 = model.blend_tiles(maps, (48, 150), 64, 32, include=include)
    side.synchronize()
    assert torch.equal(mask3, mask) and torch.equal(output3.view(torch.int32), output.view(torch.int32))


def test_blend_uncovered_pixels_and_eight_classes(torch_cuda, model):
    """No included patch over a pixel: 0 / 1e-8 = 0 and class 0.  C = 8 against the restatement, odd sizes."""
    torch = torch_cuda
    r = np.random.default_rng(5)
    H, W = 67, 131                                            # 3 blocks wide, 17 high, neither a multiple of the block
    plan = tl.tile_plan(H, W, 64, 32)
    maps = r.standard_normal((plan.n_patches, 8, 16, 16)).astype(np.float32)
    inc = r.random(plan.n_patches) < 0.5
    inc[0] = False                                            # the top-left corner is covered by patch 0 alone
    want_mask, want = tl.blend_tiles_np(maps, plan, H, W, 64, include=inc)
    assert not want[0, 0].any()
    mask, output = model.blend_tiles(torch.from_numpy(maps).cuda(), (H, W), 64, 32, include=torch.from_numpy(inc.astype(np.uint8)).cuda())
    assert np.array_equal(bits(output[0].cpu().numpy()), bits(want)) and np.array_equal(mask[0].cpu().numpy(), want_mask)


# ---- 2. the gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_gather_equals_restatement_and_reference_input(torch_cuda, model, syn, tag):
    torch = torch_cuda
    c = CASES[TAGS.index(tag)]
    img = frame_rgb(syn, c)
    other = np.ascontiguousarray(syn.make_frame_u8(c["H"], c["W"], c["index"] + 100, "uniform", c["seed"]))
    plan = tl.tile_plan(c["H"], c["W"], c["patch"], c["stride"])
    frames = torch.from_numpy(np.stack([img, other])).cuda()                       # B = 2, two different frames
    for order in ("rgb", "bgr"):
        got = model.gather_tiles(frames, c["patch"], c["stride"], c["target"], order).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == (2 * plan.n_patches, c["target"], c["target"], 3)
        for i, f in enumerate((img, other)):
            want = tl.gather_tiles_np(f, plan, c["patch"], c["target"], order)
            assert np.array_equal(got[i * plan.n_patches:(i + 1) * plan.n_patches], want), (tag, order, i)
        if order == "rgb":                                    # the bytes the reference fed its network (RGB there, BGR here)
            assert sha(got[:plan.n_patches][..., ::-1]) == c["fed_sha"], tag
    again = model.gather_tiles(frames, c["patch"], c["stride"], c["target"], "bgr").cpu().numpy()
    assert np.array_equal(again, got)


def test_gather_identity_at_equal_size(torch_cuda, model, syn):
    torch = torch_cuda
    img = syn.make_frame_u8(64, 96, 9, "uniform", 77)
    got = model.gather_tiles(torch.from_numpy(img[None]).cuda(), 64, 32, 64, "bgr").cpu().numpy()
    assert np.array_equal(got[0], img[:, :64]) and np.array_equal(got[1], img[:, 32:])


# ---- 3. the gate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_gate_scores_are_the_maximum(torch_cuda, model, tag):
    torch = torch_cuda
    c = CASES[TAGS.index(tag)]
    maps = G[tag + "_maps"]
    for cls in range(c["C"]):
        want = maps[:, cls].reshape(len(maps), -1).max(axis=1)
        thr = float(np.sort(want)[len(want) // 2])            # a score itself: >= keeps it
        include, scores = model.tile_gate(torch.from_numpy(maps).cuda(), thr, cls)
        assert np.array_equal(bits(scores.cpu().numpy()), bits(want)), (tag, cls)
        assert np.array_equal(include.cpu().numpy().astype(bool), want >= np.float32(thr)), (tag, cls)
    if c["thr"] is not None:
        include, scores = model.tile_gate(torch.from_numpy(maps).cuda(), c["thr"], c["gate_class"])
        assert np.array_equal(scores.cpu().numpy(), G[tag + "_scores"])
        assert np.array_equal(include.cpu().numpy().astype(bool), stored_include(c))


# ---- 4. end to end: the engine's network between gather and blend ----------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_predict_tiled_end_to_end(torch_cuda, trained, syn, tag):
    """predict_tiled in `exact` with the fixtures' weights against the reference's stored results.  Bilinear sampling
    and averaging are convex combinations and softmax does not expand differences, so the network's 1e-3 logit bar
    carries over to `output`.  Masks must agree wherever the stored top-two margin is at least 2e-3 (twice the bar)."""
    torch = torch_cuda
    c = CASES[TAGS.index(tag)]
    m = trained[c["C"]]
    frames = torch.from_numpy(frame_rgb(syn, c)[None]).cuda()
    mask, output = m.predict_tiled(frames, c["patch"], c["stride"], c["target"], blend=c["blend"], gate_thr=c["thr"],
                                   gate_class=c["gate_class"], channel_order="rgb")
    want, want_mask = G[tag + "_output"], G[tag + "_mask"]
    if c["thr"] is not None:                                  # every gate decision, from the parts
        probs = m.predict_proba(m.gather_tiles(frames, c["patch"], c["stride"], c["target"], "rgb")[:4])
        include, scores = m.tile_gate(probs, c["thr"], c["gate_class"])
        print(f"{tag}: max|dscore| = {np.abs(scores.cpu().numpy() - G[tag + '_scores']).max():.3e}")
        assert np.array_equal(include.cpu().numpy().astype(bool), stored_include(c)), tag
    err = float(np.abs(output[0].cpu().numpy() - want).max())
    top = np.sort(want, axis=-1)
    sure = (top[..., -1] - top[..., -2]) >= 2e-3
    wrong = int(((mask[0].cpu().numpy() != want_mask) & sure).sum())
    print(f"{tag}: max|doutput| = {err:.3e}, excluded pixels = {1 - sure.mean():.4f}, mask mismatches outside them = {wrong}")
    assert err < 1e-3, tag
    assert 1 - sure.mean() <= 0.01, tag
    assert wrong == 0, tag
    # the BGR frame with channel_order="bgr" is the same call
    mask_b, output_b = m.predict_tiled(frames.flip(-1).contiguous(), c["patch"], c["stride"], c["target"], blend=c["blend"],
                                       gate_thr=c["thr"], gate_class=c["gate_class"], channel_order="bgr")
    assert torch.equal(mask_b, mask) and torch.equal(output_b.view(torch.int32), output.view(torch.int32))


def test_predict_tiled_arguments_and_empty_plan(torch_cuda, trained):
    torch = torch_cuda
    m = trained[2]
    frames = torch.zeros((2, 32, 150, 3), dtype=torch.uint8, device="cuda")
    mask, output = m.predict_tiled(frames, 64, 32, 32)                             # (32 - 64) % 32 == 0: no patch, zeros
    assert tuple(mask.shape) == (2, 32, 150) and not mask.any() and tuple(output.shape) == (2, 32, 150, 2) and not output.any()
    ok = torch.zeros((1, 100, 150, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        m.predict_tiled(ok, 64, 32, 40)                                            # target_size not a multiple of 16
    with pytest.raises(ValueError):
        m.predict_tiled(ok, 64, 0, 32)
    with pytest.raises(ValueError):
        m.predict_tiled(ok, 64, 32, 32, blend="mean")
    with pytest.raises(ValueError):
        m.predict_tiled(ok, 64, 32, 32, blend="logits", gate_thr=0.5)
    with pytest.raises(ValueError):
        m.predict_tiled(ok, 64, 32, 32, channel_order="gbr")
    with pytest.raises(RuntimeError):
        m.predict_tiled(ok.cpu(), 64, 32, 32)
    with pytest.raises(RuntimeError):
        m.predict_tiled(ok[..., :2], 64, 32, 32)
    with pytest.raises(ValueError):                                                # a pad of the axis length or more
        m.predict_tiled(torch.zeros((1, 20, 150, 3), dtype=torch.uint8, device="cuda"), 64, 64, 32)


def test_simple_unet_has_the_same_surface(torch_cuda):
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    m = SimpleUNet(3).to("cuda:0")
    r = np.random.default_rng(3)
    plan = tl.tile_plan(70, 90, 64, 32)
    maps = r.standard_normal((plan.n_patches, 3, 24, 24)).astype(np.float32)
    want_mask, want = tl.blend_tiles_np(maps, plan, 70, 90, 64)
    mask, output = m.blend_tiles(torch.from_numpy(maps).cuda(), (70, 90), 64, 32)
    assert np.array_equal(bits(output[0].cpu().numpy()), bits(want)) and np.array_equal(mask[0].cpu().numpy(), want_mask)


# ---- 5. the C ABI's error returns: an error code, and no kernel ---------------------------------------------------------------
def test_c_abi_error_returns(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    model.blend_tiles(torch.zeros((2, 3, 16, 16), device="cuda"), (64, 96), 64, 32)           # makes sure the engine exists
    h = model._handle
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    err = lambda: lib.unetpp_last_error(h).decode()
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    H, W = 64, 96
    ys_a, xs_a, far_a = np.array([0], np.int32), np.array([0, 32], np.int32), np.array([64], np.int32)      # kept alive below
    ys, xs, far = ptr(ys_a), ptr(xs_a), ptr(far_a)
    frames = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
    patches = torch.full((2, 32, 32, 3), 7, dtype=torch.uint8, device="cuda")
    maps = torch.zeros((2, 9, 32, 32), device="cuda")
    mask = torch.full((1, H, W), 7, dtype=torch.uint8, device="cuda")
    scores = torch.full((2,), 7.0, device="cuda")
    include = torch.full((2,), 7, dtype=torch.uint8, device="cuda")

    def gather(frames_=frames, patches_=patches, ys_=ys, xs_=xs, hh=H, t=32, order=1, patch=64, ny=1):
        return lib.unetpp_tile_gather_u8(h, p(frames_), 1, hh, W, ys_, ny, xs_, 2, patch, t, order, p(patches_), None)

    def blend(maps_=maps, mask_=mask, classes=3, ys_=ys, xs_=xs, ny=1):
        return lib.unetpp_tile_blend_f32(h, p(maps_), 1, classes, 32, ys_, ny, xs_, 2, 64, None, H, W, p(mask_), None, None)

    def gate(maps_=maps, scores_=scores, include_=include, cls=1):
        return lib.unetpp_tile_gate_f32(h, p(maps_), 2, 3, 32, cls, 0.5, p(scores_), p(include_), None)

    assert gather(frames_=None) == -1 and "null" in err()
    assert gather(patches_=None) == -1 and gather(ys_=None) == -1 and gather(xs_=None) == -1
    assert gather(hh=32) == -2 and "reflect padding" in err()                 # a 64 patch on 32 rows: padding of H
    assert gather(hh=20) == -2
    assert gather(t=30) == -1 and gather(order=2) == -1 and gather(ny=0) == -1 and gather(ny=65) == -2
    assert gather(ys_=far) == -1 and "origin" in err()
    assert lib.unetpp_tile_gather_u8(None, p(frames), 1, H, W, ys, 1, xs, 2, 64, 32, 1, p(patches), None) == -1
    assert blend(maps_=None) == -1 and "null" in err()
    assert blend(mask_=None) == -1 and blend(ys_=None) == -1 and blend(xs_=None) == -1
    assert blend(classes=9) == -2 and "classes" in err()
    assert blend(classes=0) == -1 and blend(ny=65) == -2 and blend(ys_=far) == -1
    assert gate(maps_=None) == -1 and gate(scores_=None) == -1 and gate(include_=None) == -1
    assert gate(cls=3) == -1 and "gate_class" in err() and gate(cls=-1) == -1
    torch.cuda.synchronize()
    # no kernel ran: nothing was written
    assert (patches == 7).all() and (mask == 7).all() and (scores == 7).all() and (include == 7).all()
    assert gather() == 0 and blend() == 0 and gate() == 0
    torch.cuda.synchronize()
    assert not patches.any() and not mask.any() and not include.any() and not scores.any()
    del ys_a, xs_a, far_a
