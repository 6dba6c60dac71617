"""Stage-2 burr detection on the device (unetpp_gray_u8, unetpp_gaussian_blur_u8, unetpp_canny_u8,
unetpp_laplacian_band_u8, unetpp_components_filter_box and the NestedUNet methods built on them) against the NumPy
restatement (unet_amd/edges.py) and the fixtures made from the reference's own functions
(tests/golden/burr_scenes.npz).  Everything is integer arithmetic: exact equality, no tolerance.
Run on the GPU box:  python -m pytest tests/test_gpu_burr.py -m gpu"""
import ctypes
import hashlib
import math

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import components as cc
from unet_amd import edges as ed

pytestmark = pytest.mark.gpu

BLURS = (None, (3, 1.0), (5, 1.0), (7, 2.0))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: none of this needs any


@pytest.fixture(scope="module")
def tile():
    """(core rows, core columns) of one workgroup of the Canny kernel, from the library."""
    from unet_amd import _lib
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().unetpp_canny_layout(512, 512, ctypes.byref(rows), ctypes.byref(cols)) == 0
    assert rows.value >= 8 and cols.value >= 16
    return rows.value, cols.value


def canny_ref(frames, low, high, blur):
    t = None if blur is None else ed.gaussian_taps(*blur)
    return np.stack([ed.canny_np(f if t is None else ed.gaussian_blur_np(f, t), low, high) for f in frames])


# ---- 1. the fixtures from the reference's own functions ----------------------------------------------------------------
def test_fixture_cases_through_the_public_methods(torch_cuda, model):
    torch = torch_cuda
    g = load_golden("burr_scenes")
    rows = [tuple(r) for r in g["cases"].tolist()]
    scenes = sorted({(int(H), int(W), int(seed)) for _, kind, H, W, seed, _, _ in rows if kind in ("detect", "rulebased")})
    assert len(scenes) == 3
    seen = 0
    for H, W, seed in scenes:
        grey, cable = ed.make_burr_scene(H, W, seed)
        unpack = lambda tag: np.unpackbits(g[tag + "_out"])[:H * W].reshape(H, W)
        mine = [r for r in rows if r[1] in ("detect", "rulebased") and (int(r[2]), int(r[3]), int(r[4])) == (H, W, seed)]
        assert len(mine) == 5 and all(r[6] == hashlib.sha256(np.stack([grey, cable]).tobytes()).hexdigest() for r in mine)
        # once the frame alone, once in a batch between an empty-cable frame and a second copy
        for batch in (1, 3):
            dg = torch.from_numpy(np.stack([grey] * batch)).cuda()
            cab = np.stack([cable] * batch)
            if batch == 3:
                cab[1] = 0
            dc = torch.from_numpy(cab).cuda()
            for tag, kind, _, _, _, param, _ in mine:
                if kind == "detect":
                    p = ed.PRESETS[param]
                    got = model.detect_burrs(dg, dc, min_area=p["min_area"], max_area=p["max_area"]).cpu().numpy()
                    ref = unpack(tag)                                       # the reference's burr mask is 0 / 1
                else:
                    got = model.burr_mask_rulebased(dg, dc * int(param)).cpu().numpy()
                    ref = unpack(tag) * np.uint8(255)
                assert got.dtype == np.uint8 and got.shape == (batch, H, W)
                for i in range(batch):
                    want = np.zeros_like(ref) if (batch == 3 and i == 1) else ref   # an empty cable: the early returns
                    assert np.array_equal(got[i], want), (tag, batch, i)
                seen += 1
    assert seen == 30
    # the tail on prepared rectangles: side and aspect clauses on the reference's own loop
    edges, cable = ed.make_crafted_burr_case()
    H, W = edges.shape
    crafted = [r for r in rows if r[1] == "crafted"]
    assert len(crafted) == 2
    de, dc = torch.from_numpy(np.stack([edges, edges])).cuda(), torch.from_numpy(np.stack([cable, cable])).cuda()
    for tag, _, h, w, _, param, sha in crafted:
        assert (int(h), int(w)) == (H, W) and sha == hashlib.sha256(np.stack([edges, cable]).tobytes()).hexdigest()
        p = ed.PRESETS[param]
        got = model.burrs_from_edges(de, dc, min_area=p["min_area"], max_area=p["max_area"]).cpu().numpy()
        ref = np.unpackbits(g[tag + "_out"])[:H * W].reshape(H, W)
        assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref), tag


# ---- 2. blur and Canny against the restatement at the tile's seams ---------------------------------------------------
def seam_frames(H, W, th, tw, seed):
    """Three different frames: noise, a smooth ramp, and steps lying exactly on a tile seam and on each image border."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    noise = r.integers(0, 256, (H, W), dtype=np.uint8)
    ramp = ((3 * x + 5 * y) % 256).astype(np.uint8) // 2 + (60 * np.sin(x / 7.0) * np.cos(y / 5.0) + 60).astype(np.uint8)
    steps = np.full((H, W), 90, np.uint8)
    steps[min(th, H - 3):, :] += 40                              # a horizontal step on the first row seam
    steps[:, min(tw, W - 3):] += 60                              # a vertical step on the first column seam
    steps[0, :] = 200; steps[H - 1, :] = 10; steps[:, 0] = 15; steps[:, W - 1] = 220    # steps on each image border
    steps[1, W // 2:] = 0; steps[H // 2:, 1] = 255
    return np.stack([noise, ramp, steps])


def seam_shapes(th, tw):
    return [(8, 8), (9, 17), (th, tw), (th - 1, tw - 1), (th + 1, tw + 1), (th - 1, tw + 1), (th + 1, tw - 1), (2 * th + 3, 3 * tw + 5)]


def test_gaussian_blur_matches_restatement_at_the_seams(torch_cuda, model, tile):
    torch = torch_cuda
    for H, W in seam_shapes(*tile):
        frames = seam_frames(H, W, *tile, seed=H * 1000 + W)
        d = torch.from_numpy(frames).cuda()
        for ksize, sigma in BLURS[1:]:
            t = ed.gaussian_taps(ksize, sigma)
            ref = np.stack([ed.gaussian_blur_np(f, t) for f in frames])
            assert np.array_equal(model.gaussian_blur(d, ksize, sigma).cpu().numpy(), ref), (H, W, ksize)
        skew = np.array([0, 3, 200, 50, 3], np.int32)            # caller-supplied taps need not be symmetric
        ref = np.stack([ed.gaussian_blur_np(f, skew) for f in frames])
        assert np.array_equal(model.gaussian_blur(d, taps=skew).cpu().numpy(), ref), (H, W, "skew")


def test_canny_matches_restatement_at_the_seams(torch_cuda, model, tile):
    torch = torch_cuda
    for H, W in seam_shapes(*tile):
        frames = seam_frames(H, W, *tile, seed=H * 1000 + W)
        d = torch.from_numpy(frames).cuda()
        for blur in BLURS:
            for low, high in ((50, 150), (200.9, 400.2)) if blur is None else ((50, 150), (20, 60)):
                got = model.canny(d, low, high, blur=blur).cpu().numpy()
                ref = canny_ref(frames, low, high, blur)
                assert got.dtype == np.uint8 and np.array_equal(got, ref), (H, W, blur, low, high)
                assert ref[0].any() or blur is not None
        # taps given as an array are the same kernel; low > high swaps
        t5 = ed.gaussian_taps(5, 1.0)
        assert torch.equal(model.canny(d, 150, 50, blur=t5), model.canny(d, 50, 150, blur=(5, 1.0)))


# ---- 3. hysteresis adversaries ----------------------------------------------------------------------------------------
def test_hysteresis_adversaries(torch_cuda, model, tile):
    torch = torch_cuda
    th, tw = tile
    adv = ed.make_hysteresis_adversaries(th, tw)
    names = sorted(adv)
    frames = np.stack([adv[n] for n in names])
    got = dict(zip(names, model.canny(torch.from_numpy(frames).cuda(), 50, 150).cpu().numpy()))
    for n in names:
        assert np.array_equal(got[n], ed.canny_np(adv[n], 50, 150)), n
    # a weak serpentine over >= 6 tiles with its strong pixels at one end: all of it is kept
    cmap = ed.canny_map_np(adv["serpentine_seeded"], 50, 150)
    ys, xs = np.nonzero(got["serpentine_seeded"])
    assert len(set(zip((ys // th).tolist(), (xs // tw).tolist()))) >= 6
    sy, sx = np.nonzero(cmap == 2)
    assert 1 <= len(sy) <= 16 and sy.max() < th and sx.max() < tw          # the seed sits in one tile, at one end
    assert np.array_equal(got["serpentine_seeded"] != 0, cmap != 0) and (cmap != 0).sum() > 3000
    # the same chain without the seed: nothing is kept
    assert (ed.canny_map_np(adv["serpentine_unseeded"], 50, 150) == 1).sum() > 3000 and not got["serpentine_unseeded"].any()
    # two chains one pixel apart diagonally, across a tile corner: only the seeded one
    cmap = ed.canny_map_np(adv["diagonal_pair"], 50, 150)
    labels, stats, _ = cc.components_np(cmap, 8, -1)
    assert len(stats) == 3 and cmap[th - 2, tw - 2] and cmap[th, tw] and labels[th - 2, tw - 2] != labels[th, tw]
    assert np.array_equal(got["diagonal_pair"] != 0, labels == labels[th - 2, tw - 2])


def test_direction_cases(torch_cuda, model):
    torch = torch_cuda
    frames = ed.make_direction_cases()
    got = model.canny(torch.from_numpy(frames).cuda(), 50, 150).cpu().numpy()
    seen = {"horizontal": 0, "vertical": 0, "diagonal+": 0, "diagonal-": 0}
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], ed.canny_np(f, 50, 150)), i
        dx, dy = ed.sobel_np(f)
        x, y = np.abs(dx), np.abs(dy) << 15
        hz = y < x * ed.TG22
        vt = ~hz & (y > x * ed.TG22 + (x << 16))
        kept = got[i] != 0
        seen["horizontal"] += int((kept & hz).sum()); seen["vertical"] += int((kept & vt).sum())
        seen["diagonal+"] += int((kept & ~hz & ~vt & ((dx ^ dy) >= 0)).sum())
        seen["diagonal-"] += int((kept & ~hz & ~vt & ((dx ^ dy) < 0)).sum())
    assert min(seen.values()) >= 100, seen


# ---- 4. the Laplacian band and the uint8 wrap ---------------------------------------------------------------------------
def test_rulebased_wraps_the_laplacian_like_the_reference(torch_cuda, model):
    torch = torch_cuda
    H, W = 40, 72
    grey = np.zeros((H, W), np.uint8)
    cable = np.zeros((H, W), np.uint8)
    cable[:, 30:34] = 1                                          # band_out = 10: columns 20..29 and 34..43
    grey[5, 22] = 255                                            # |lap| = 1020 -> 252
    grey[10, 22] = 75                                            # 300 -> 44
    grey[15, 22] = 64                                            # 256 -> 0
    grey[20, 21] = 100; grey[20, 23] = 100; grey[19, 22] = 55    # (20, 22): 255 -> 255
    grey[25, 50] = 255                                           # outside the band
    grey[0, 25] = 200; grey[H - 1, 40] = 90                      # on the image border: reflected rows
    lap = np.abs(ed.laplacian_np(grey))
    assert [int(lap[5, 22]), int(lap[10, 22]), int(lap[15, 22]), int(lap[20, 22])] == [1020, 300, 256, 255]
    dg, dc = torch.from_numpy(grey[None]).cuda(), torch.from_numpy(cable[None]).cuda()
    for thr in (30, 43, 44, 251, 252, 254, 255, 0):
        got = model.burr_mask_rulebased(dg, dc, laplacian_threshold=thr, min_area=1, max_area=500).cpu().numpy()[0]
        assert np.array_equal(got, ed.burr_mask_rulebased_np(grey, cable, laplacian_threshold=thr, min_area=1, max_area=500)), thr
        assert got[5, 22] == (255 if 252 > thr else 0) and got[10, 22] == (255 if 44 > thr else 0) and got[15, 22] == 0
        assert got[20, 22] == (255 if 255 > thr else 0) and got[25, 50] == 0
    # odd width, masks as 0/255, class matching
    r = np.random.default_rng(5)
    grey = r.integers(0, 256, (3, 37, 53), dtype=np.uint8)
    cable = np.zeros((3, 37, 53), np.uint8)
    cable[0, 10:20, 20:30] = 255; cable[1, :, 25] = 255; cable[2, 5:30, 5:9] = 2; cable[2, 0:3, 40:50] = 1
    for match, band_out in ((-1, 10), (2, 3), (255, 6)):
        got = model.burr_mask_rulebased(torch.from_numpy(grey).cuda(), torch.from_numpy(cable).cuda(), match, band_out=band_out,
                                        laplacian_threshold=120, min_area=2, max_area=40, out_value=7).cpu().numpy()
        ref = np.stack([ed.burr_mask_rulebased_np(grey[i], cable[i], match, band_out=band_out, laplacian_threshold=120, min_area=2,
                                                  max_area=40, out_value=7) for i in range(3)])
        assert np.array_equal(got, ref), (match, band_out)
    assert ref.any()


# ---- 5. the box rule at its clause boundaries --------------------------------------------------------------------------
def test_filter_components_box_at_each_clause_boundary(torch_cuda, model):
    torch = torch_cuda
    rects = [(5, 6), (29, 1), (1, 29), (6, 5), (4, 8), (31, 1), (3, 10), (10, 2), (2, 10), (4, 20), (20, 4), (4, 19), (4, 21), (7, 35),
             (7, 34), (28, 28), (20, 40), (20, 41), (25, 32), (3, 3), (4, 4), (3, 12), (1, 1)]
    m = np.zeros((2, 160, 333), np.uint8)
    x = y = 2; row_h = 0
    for h, w in rects:
        if x + w + 2 > 333:
            x = 2; y += row_h + 2; row_h = 0
        m[0, y:y + h, x:x + w] = 3
        x += w + 2; row_h = max(row_h, h)
    assert y + row_h < 160
    m[1] = m[0, ::-1, ::-1]                                      # a second, different frame
    m[1, 100:140, 200:220] = 3
    d = torch.from_numpy(m).cuda()
    cases = [(30, 800, 5.0, 3), (31, 799, 5.0, 3), (30, 800, 4.999999, 3), (30, 800, 4.9999985, 3), (20, 500, math.inf, 0), (1, 10 ** 9, 5.000001, 0),
             (29.5, 800.5, 10.0, 3.5), (0, 0, 5.0, 3)]
    kept_counts = set()
    for min_area, max_area, max_aspect, min_side in cases:
        got = model.filter_components_box(d, 3, min_area, max_area, max_aspect, min_side, out_value=9).cpu().numpy()
        ref = np.stack([ed.filter_box_np(f, 3, min_area, max_area, max_aspect, min_side, 9) for f in m])
        assert np.array_equal(got, ref), (min_area, max_area, max_aspect, min_side)
        kept_counts.add(int((ref != 0).sum()))
    assert len(kept_counts) == len(cases)                        # every clause boundary changes what is kept
    # 4 x 20: aspect = 20 / (4 + 1e-6) = 4.99999875...: the 1e-6 of the reference decides, in fp64
    _, stats, _ = cc.components_np(m[0], 8, 3)
    assert ed.keep_box(stats, 1, 10 ** 9, 4.999999, 0).sum() == ed.keep_box(stats, 1, 10 ** 9, 4.9999985, 0).sum() + 2


def test_bgr_to_gray(torch_cuda, model):
    torch = torch_cuda
    r = np.random.default_rng(11)
    frames = r.integers(0, 256, (2, 19, 23, 3), dtype=np.uint8)
    frames[0, 0, :16] = np.array([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1], [254, 255, 255], [128, 128, 128]] * 2)
    got = model.bgr_to_gray(torch.from_numpy(frames).cuda()).cpu().numpy()
    assert np.array_equal(got, ed.bgr_to_gray_np(frames))
    assert got[0, 0, 0] == 255 and got[0, 0, 1] == 0 and got[0, 0, 7] == 128


# ---- 6. determinism and limits --------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_and_on_a_second_stream(torch_cuda, model, tile):
    torch = torch_cuda
    th, tw = tile
    r = np.random.default_rng(3)
    frames = r.integers(0, 256, (3, 2 * th + 3, 3 * tw + 5), dtype=np.uint8)    # noise: thousands of weak fragments
    grey, cable = ed.make_burr_scene(96, 200, 2)
    d = torch.from_numpy(frames).cuda()
    dg, dc = torch.from_numpy(grey[None]).cuda(), torch.from_numpy(cable[None]).cuda()
    first = model.canny(d, 100, 300, blur=(3, 1.0))
    burrs = model.detect_burrs(dg, dc)
    assert first.any() and burrs.any()
    for _ in range(3):
        assert torch.equal(model.canny(d, 100, 300, blur=(3, 1.0)), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again, burrs2 = model.canny(d, 100, 300, blur=(3, 1.0)), model.detect_burrs(dg, dc)
    side.synchronize()
    assert torch.equal(again, first) and torch.equal(burrs2, burrs)


def test_limits_raise_before_any_launch(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    small = torch.zeros((1, 7, 40), dtype=torch.uint8, device="cuda:0")
    ok = torch.zeros((1, 8, 40), dtype=torch.uint8, device="cuda:0")
    for call in (lambda: model.canny(small, 50, 150), lambda: model.gaussian_blur(small), lambda: model.detect_burrs(small, small),
                 lambda: model.canny(ok.transpose(1, 2)[:, :, :7], 50, 150)):
        with pytest.raises(ValueError, match="8 <= H, W"):
            call()
    for taps in ([14, 62, 104, 62, 15], [128, 128], [256, 0, 0, 0, 0, 0, 0, 0, 0], [-1, 258, -1]):
        with pytest.raises(ValueError, match="taps|tap"):
            model.canny(ok, 50, 150, blur=np.array(taps, np.int32))
        with pytest.raises(ValueError, match="taps|tap"):
            model.detect_burrs(ok, ok, taps=np.array(taps, np.int32))
    # the C ABI refuses the same and leaves the output alone
    lib = _lib.load()
    model.canny(ok, 50, 150)                                     # makes the engine
    out = torch.full((1, 8, 40), 7, dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(int(lib.unetpp_canny_workspace_bytes(1, 8, 40)), dtype=torch.uint8, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    taps = lambda *v: (ctypes.c_int32 * len(v))(*v)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.unetpp_canny_workspace_bytes(1, 7, 40) == 0 and lib.unetpp_canny_workspace_bytes(1, 8, 40) >= 8 * 40 * 6
    assert lib.unetpp_canny_u8(model._handle, p(ok), 1, 7, 40, None, 0, 50.0, 150.0, p(out), p(ws), stream) == -2
    assert lib.unetpp_canny_u8(model._handle, p(ok), 1, 8, 40, taps(14, 62, 104, 62, 15), 5, 50.0, 150.0, p(out), p(ws), stream) == -1
    assert lib.unetpp_canny_u8(model._handle, p(ok), 1, 8, 40, taps(*([28] * 8 + [32])), 9, 50.0, 150.0, p(out), p(ws), stream) == -2
    assert lib.unetpp_canny_u8(model._handle, p(ok), 1, 8, 40, taps(128, 128), 2, 50.0, 150.0, p(out), p(ws), stream) == -1
    assert lib.unetpp_gaussian_blur_u8(model._handle, p(ok), 1, 7, 40, taps(256), 1, p(out), stream) == -2
    assert lib.unetpp_gaussian_blur_u8(model._handle, p(ok), 1, 8, 40, taps(100, 100, 100), 3, p(out), stream) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all())
