"""The multi-scale and the DoG burr detector on the device (unetpp_edges_union_u8, unetpp_dog_band_u8,
unetpp_count_nonzero_u8 and the NestedUNet methods built on them) against the NumPy restatement (unet_amd/edges.py) and
the fixtures made from the reference's own functions (tests/golden/burr_enhanced_scenes.npz).  Integer arithmetic and
one correctly rounded float64 expression: exact equality, no tolerance.
Run on the GPU box:  python -m pytest tests/test_gpu_burr_enhanced.py -m gpu"""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import edges as ed
from unet_amd import morphology as mo

pytestmark = pytest.mark.gpu

TH, TW = 32, 128          # the tile of the kernels; test_tile_is_the_canny_tile checks it against the library
SEAM_SHAPES = [(8, 8), (9, 17), (TH, TW), (TH - 1, TW - 1), (TH + 1, TW + 1), (TH - 1, TW + 1), (TH + 1, TW - 1), (2 * TH + 3, 3 * TW + 5)]


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
def golden():
    g = load_golden("burr_enhanced_scenes")
    return g, [tuple(r) for r in g["cases"].tolist()]


def seam_frames(H, W, seed):
    """Three different frames: noise, a smooth ramp, and steps lying exactly on a tile seam and on each image border
    (where the reflect-101 of these operators and the replicate of Canny's Sobel part ways)."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    noise = r.integers(0, 256, (H, W), dtype=np.uint8)
    ramp = ((3 * x + 5 * y) % 256).astype(np.uint8) // 2 + (60 * np.sin(x / 7.0) * np.cos(y / 5.0) + 60).astype(np.uint8)
    steps = np.full((H, W), 90, np.uint8)
    steps[min(TH, H - 3):, :] += 40                              # a horizontal step on the first row seam
    steps[:, min(TW, W - 3):] += 60                              # a vertical step on the first column seam
    steps[0, :] = 200; steps[H - 1, :] = 10; steps[:, 0] = 15; steps[:, W - 1] = 220    # steps on each image border
    steps[1, W // 2:] = 0; steps[H // 2:, 1] = 255
    return np.stack([noise, ramp, steps])


def union_ref(frames, canny, sthr=50, lthr=15):
    return np.stack([ed.edges_combined_np(f, c, sthr, lthr) for f, c in zip(frames, canny)])


def sobel_only(model, torch, frames, thr=50):
    """The Sobel source alone: an empty Canny image and a Laplacian threshold nothing passes."""
    d = torch.from_numpy(frames).cuda()
    return model.edges_combined(d, torch.zeros_like(d), sobel_threshold=thr, laplacian_threshold=255).cpu().numpy()


def test_tile_is_the_canny_tile():
    from unet_amd import _lib
    rows, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().unetpp_canny_layout(512, 512, ctypes.byref(rows), ctypes.byref(cols)) == 0
    assert (rows.value, cols.value) == (TH, TW)


# ---- 1. the fixtures from the reference's own functions ----------------------------------------------------------------
@pytest.mark.parametrize("index", range(3))
def test_fixture_scenes_through_the_public_methods(torch_cuda, model, golden, index):
    torch = torch_cuda
    g, rows = golden
    tag, _, H, W, seed, sigma, sha = [r for r in rows if r[1] == "enhanced"][index]
    H, W, seed = int(H), int(W), int(seed)
    unpack = lambda t: np.unpackbits(g[t + "_out"])[:H * W].reshape(H, W)
    grey, cable = ed.make_burr_scene(H, W, seed, noise_sigma=float(sigma))
    assert sha == hashlib.sha256(np.stack([grey, cable]).tobytes()).hexdigest()
    # once the frame alone, once in a batch between an empty-cable frame and a second copy
    for batch in (1, 3):
        cab = np.stack([cable] * batch)
        if batch == 3:
            cab[1] = 0
        got = model.detect_burrs_enhanced(torch.from_numpy(np.stack([grey] * batch)).cuda(), torch.from_numpy(cab).cuda()).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == (batch, H, W)
        for i in range(batch):
            want = np.zeros((H, W), np.uint8) if (batch == 3 and i == 1) else unpack(tag)      # an empty cable: the early returns
            assert np.array_equal(got[i], want), (tag, batch, i)
    dogs = [r for r in rows if r[1] == "dog" and (int(r[2]), int(r[3]), int(r[4])) == (H, W, seed)]
    assert len(dogs) == 2
    grey, cable = ed.make_burr_scene(H, W, seed)
    dg = torch.from_numpy(np.stack([grey] * 3)).cuda()
    cab = np.stack([cable] * 3); cab[1] = 0
    for tag, _, _, _, _, scale, sha in dogs:
        assert sha == hashlib.sha256(np.stack([grey, cable]).tobytes()).hexdigest()
        mask = model.burr_mask_dog(dg, torch.from_numpy(cab * np.uint8(int(scale))).cuda())
        got = mask.cpu().numpy()
        ref = unpack(tag) * np.uint8(255)
        assert got.dtype == np.uint8 and np.array_equal(got[0], ref) and not got[1].any() and np.array_equal(got[2], ref), tag
        assert model.has_burr(mask).cpu().tolist() == [True, False, True]


def test_fixture_crafted_tail(torch_cuda, model, golden):
    torch = torch_cuda
    g, rows = golden
    (tag, _, H, W, _, _, sha), = [r for r in rows if r[1] == "crafted"]
    grey, edges, cable = ed.make_crafted_enhanced_case()
    assert (int(H), int(W)) == edges.shape and sha == hashlib.sha256(np.stack([grey, edges, cable]).tobytes()).hexdigest()
    ref = np.unpackbits(g[tag + "_out"])[:edges.size].reshape(edges.shape)
    dg, de, dc = (torch.from_numpy(np.stack([a, a])).cuda() for a in (grey, edges, cable))
    combined = model.edges_combined(dg, de)
    assert np.array_equal(combined.cpu().numpy()[1], ed.edges_combined_np(grey, edges)) and torch.equal(de[0], torch.from_numpy(edges).cuda())
    got = model.burrs_from_edges(combined, dc, min_area=50, max_area=500, band_ksize=25, close_ksize=5, open_ksize=3, max_aspect=6.0,
                                 min_side=4).cpu().numpy()
    assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref) and ref.any()


# ---- 2. the edge union against the restatement at the tile's seams -----------------------------------------------------
@pytest.mark.parametrize("shape", SEAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edges_combined_matches_restatement_at_the_seams(torch_cuda, model, shape):
    torch = torch_cuda
    H, W = shape
    frames = seam_frames(H, W, seed=H * 1000 + W)
    r = np.random.default_rng(H + W)
    canny = (r.random((3, H, W)) < 0.05).astype(np.uint8) * np.uint8(255)
    d, dc = torch.from_numpy(frames).cuda(), torch.from_numpy(canny).cuda()
    for sthr, lthr in ((50, 15), (10, 100), (200.5, 254), (-1, 255), (255, -1), (255, 255)):
        got = model.edges_combined(d, dc, sobel_threshold=sthr, laplacian_threshold=lthr).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, union_ref(frames, canny, sthr, lthr)), (H, W, sthr, lthr)
    assert torch.equal(dc, torch.from_numpy(canny).cuda())                   # a caller's Canny image is left alone
    # each source alone, so that a fault in one cannot hide behind another
    so = sobel_only(model, torch, frames)
    assert np.array_equal(so, np.stack([ed.sobel_edges_np(f) for f in frames])) and so.any() and not so.all()
    la = model.edges_combined(d, torch.zeros_like(d), sobel_threshold=255).cpu().numpy()
    assert np.array_equal(la, np.stack([ed.laplacian_edges_np(f) for f in frames])) and la.any()
    # the steps on the border: reflect-101 gives no derivative across it, Canny's replicate does
    dx, _ = ed.sobel_xy_np(frames[2]); cx, _ = ed.sobel_np(frames[2])
    assert not dx[:, 0].any() and cx[:, 0].any()
    # canny_edges=None runs the Canny of the reference's constants itself
    own = model.edges_combined(d).cpu().numpy()
    t = ed.gaussian_taps(5, 1.0)
    ref = union_ref(frames, [ed.canny_np(ed.gaussian_blur_np(f, t), 30, 100) for f in frames])
    assert np.array_equal(own, ref), (H, W)


# ---- 3. the per-frame maximum -------------------------------------------------------------------------------------------
def test_maximum_in_the_last_partial_tile_and_on_the_border(torch_cuda, model):
    torch = torch_cuda
    H, W = 2 * TH + 3, 3 * TW + 5
    r = np.random.default_rng(8)
    base = r.integers(100, 104, (H, W), dtype=np.uint8)                     # s of the background: a few hundred at most
    corner, border = base.copy(), base.copy()
    corner[H - 2, W - 2] = 255                                               # its response lies in the last, 3 x 5 tile only
    border[H - 1, W - 1] = 255                                               # the same on the image border
    frames = np.stack([corner, border, base])
    got = sobel_only(model, torch, frames)
    assert np.array_equal(got, np.stack([ed.sobel_edges_np(f) for f in frames]))
    for i in (0, 1):
        ys, xs = np.nonzero(got[i])
        assert 1 <= len(ys) <= 8 and ys.min() >= 2 * TH and xs.min() >= 3 * TW       # nothing but the pixel's neighbours passes
    assert got[2].sum() > 100 * 255                                          # a maximum that missed the pixel would pass the texture
    dx, dy = ed.sobel_xy_np(corner)
    s = dx.astype(np.int64) ** 2 + dy.astype(np.int64) ** 2
    assert s[:2 * TH, :].max() * 400 < s.max() and s[:, :3 * TW].max() * 400 < s.max()


def test_maxima_of_a_batch_do_not_leak_and_a_constant_frame_has_no_sobel_edges(torch_cuda, model):
    torch = torch_cuda
    H, W = TH + 5, TW + 9
    r = np.random.default_rng(9)
    faint = r.integers(100, 103, (H, W), dtype=np.uint8)                     # max s below 10^2
    mild = (100 + 12 * ((np.arange(H)[:, None] // 7 + np.arange(W)[None, :] // 5) % 2)).astype(np.uint8)     # 10^3 .. 10^4
    loud = r.integers(0, 256, (H, W), dtype=np.uint8)                        # 10^5 .. 10^6
    flat = np.full((H, W), 93, np.uint8)                                     # max s = 0
    frames = np.stack([faint, loud, flat, mild, faint[::-1].copy()])
    smax = []
    for f in frames:
        dx, dy = ed.sobel_xy_np(f)
        smax.append(int((dx.astype(np.int64) ** 2 + dy.astype(np.int64) ** 2).max()))
    assert smax[2] == 0 and 0 < smax[0] * 20 < smax[3] and smax[3] * 100 < smax[1] and len({ed.sobel_s_threshold(smax[i]) for i in (0, 1, 3)}) == 3
    for thr in (50, 120):
        got = sobel_only(model, torch, frames, thr)
        ref = np.stack([ed.sobel_edges_np(f, thr) for f in frames])
        for i in range(len(frames)):
            assert np.array_equal(got[i], ref[i]), (thr, i)
        assert not got[2].any() and all(got[i].any() for i in (0, 1, 3, 4))
        # with a neighbour's maximum the faint frames would have no edge at all, and the loud one nothing but edges
        assert not (np.sqrt(float(smax[0])) / np.sqrt(float(smax[1])) * 255 > thr)
    # the constant frame keeps its Canny and Laplacian sources (none here) and every order of the batch gives the same frames
    back = sobel_only(model, torch, frames[::-1].copy())
    assert np.array_equal(back[::-1], sobel_only(model, torch, frames))
    both = model.edges_combined(torch.from_numpy(frames).cuda()).cpu().numpy()
    assert not both[2].any() and both[1].any()


def _pattern(dx, dy):
    """A 3 x 3 neighbourhood on a zero background whose centre has the Sobel response (dx, dy), 0 <= dy <= dx of one
    parity: right neighbour, lower neighbour and, for an odd pair, the lower right corner."""
    k = dx & 1
    assert (dx - dy) % 2 == 0 and 0 <= dy <= dx
    p = np.zeros((3, 3), np.uint8)
    p[1, 2], p[2, 1], p[2, 2] = (dx - k) // 2, (dy - k) // 2, k
    return p


def test_pixels_exactly_at_the_threshold_and_one_below(torch_cuda, model):
    """dx + dy of a 3 x 3 Sobel pair is always even, so s = dx^2 + dy^2 is 0 mod 4 or 2 mod 8 and two neighbouring
    integers are never both reachable in one frame.  Two frames instead: a step of 20 grey levels (max s = 6400) puts the
    threshold at s_thr = 256 = 16^2 + 0^2, and pixels sit exactly on it; a step of 23 (max s = 8464) puts it at
    s_thr = 339, and pixels sit at 338 = 13^2 + 13^2, exactly one below."""
    torch = torch_cuda
    H, W = TH + 6, TW + 20
    frames, spots, want = [], [], []
    for step, (dx, dy), passes in ((20, (16, 0), True), (23, (13, 13), False)):
        smax = 16 * step * step
        s_thr = ed.sobel_s_threshold(smax, 50)
        assert dx * dx + dy * dy == (s_thr if passes else s_thr - 1)
        f = np.zeros((H, W), np.uint8)
        f[:, W - 6:] = step                                                  # the frame's maximum: dx = 4 step along the step
        at = [(3, 3), (TH - 1, 40), (TH, 60), (10, TW - 1), (14, TW), (TH + 3, TW + 8)]     # in each tile and on both sides of the seams
        for y, x in at:
            f[y - 1:y + 2, x - 1:x + 2] = _pattern(dx, dy)
        gx, gy = ed.sobel_xy_np(f)
        s = gx.astype(np.int64) ** 2 + gy.astype(np.int64) ** 2
        assert int(s.max()) == smax and all(int(s[y, x]) == dx * dx + dy * dy for y, x in at)
        frames.append(f); spots.append(at); want.append(255 if passes else 0)
    frames = np.stack(frames)
    got = sobel_only(model, torch, frames)
    assert np.array_equal(got, np.stack([ed.sobel_edges_np(f) for f in frames]))
    for i in (0, 1):
        assert all(got[i][y, x] == want[i] for y, x in spots[i]), i
        assert got[i][:, W - 7:W - 5].all()


# ---- 4. the difference of Gaussians inside a band ----------------------------------------------------------------------
def dog_ref(frames, band, thr, t1=None, t2=None):
    return np.stack([np.where((b != 0) & (ed.dog_u8_np(f, t1, t2) > thr), np.uint8(255), np.uint8(0)) for f, b in zip(frames, band)])


@pytest.mark.parametrize("shape", SEAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dog_band_matches_restatement_at_the_seams(torch_cuda, model, shape):
    torch = torch_cuda
    H, W = shape
    frames = seam_frames(H, W, seed=H * 1000 + W + 1)
    r = np.random.default_rng(H * W)
    band = np.zeros((3, H, W), np.uint8)
    band[0] = 255                                                            # every thread works
    band[1] = (r.random((H, W)) < 0.02) * r.integers(1, 256, (H, W))         # most threads idle inside working tiles
    band[2, :min(TH, H), :min(TW, W)] = 1                                    # one tile set beside tiles that are all zero
    band[2, H - 1, W - 1] = 7
    d, db = torch.from_numpy(frames).cuda(), torch.from_numpy(band).cuda()
    for thr in (30, 0, -1, 5.5, 254, 255):
        got = model.dog_band(d, db, threshold=thr).cpu().numpy()
        ref = dog_ref(frames, band, int(np.floor(thr)))
        assert got.dtype == np.uint8 and np.array_equal(got, ref), (H, W, thr)
    assert dog_ref(frames, band, 30)[0].any() and np.array_equal(dog_ref(frames, band, -1), np.where(band != 0, 255, 0))
    # other kernels: any odd lengths up to 7, symmetric or not, the identity included
    skew, one = np.array([0, 3, 200, 50, 3], np.int32), np.array([256], np.int32)
    for t1, t2 in ((skew, one), (one, ed.gaussian_taps(7, 2.0)), (ed.gaussian_taps(7, 2.0), ed.gaussian_taps(3, 1.0)), (ed.gaussian_taps(5, 1.0), skew)):
        got = model.dog_band(d, db, threshold=8, taps1=t1, taps2=t2).cpu().numpy()
        assert np.array_equal(got, dog_ref(frames, band, 8, t1, t2)), (H, W, len(t1), len(t2))


def test_dog_skips_idle_tiles_beside_working_ones(torch_cuda, model):
    torch = torch_cuda
    H, W = 3 * TH, 4 * TW
    frames = seam_frames(H, W, seed=77)
    band = np.zeros((3, H, W), np.uint8)
    band[0, TH:2 * TH, TW:2 * TW] = 255                                      # one working tile in the middle of idle ones
    band[1, :, ::2 * TW] = 255                                               # one column per other tile: one thread per row works
    band[1, TH - 1:TH + 1, :] = 255                                          # and two rows across every tile seam
    d, db = torch.from_numpy(frames).cuda(), torch.from_numpy(band).cuda()   # band[2] stays empty: every workgroup leaves early
    got = model.dog_band(d, db, threshold=10)
    ref = dog_ref(frames, band, 10)
    assert np.array_equal(got.cpu().numpy(), ref) and ref[0].any() and ref[1].any() and not ref[2].any()


# ---- 5. has_burr -----------------------------------------------------------------------------------------------------------
def test_has_burr_at_49_50_and_51_pixels(torch_cuda, model):
    torch = torch_cuda
    for H, W in ((37, 53), (2 * TH + 3, 3 * TW + 5), (64, 128)):            # odd, several chunks of 4096 pixels, vector loads
        r = np.random.default_rng(H)
        m = np.zeros((5, H, W), np.uint8)
        for i, n in enumerate((49, 50, 51, 0, H * W)):
            where = r.permutation(H * W)[:n]
            m[i].ravel()[where] = r.integers(1, 256, n)
            if 0 < n < H * W:
                m[i].ravel()[where[0]] = 0; m[i, H - 1, W - 1] = 1            # the last pixel of the frame counts
        d = torch.from_numpy(m).cuda()
        assert model.count_nonzero(d).cpu().tolist() == [49, 50, 51, 0, H * W]
        got = model.has_burr(d)
        assert got.dtype == torch.bool and got.is_cuda and got.cpu().tolist() == [False, True, True, False, True]
        assert got.cpu().tolist() == [ed.has_burr_np(f) for f in m]
        assert model.has_burr(d, 51).cpu().tolist() == [False, False, True, False, True]
        assert model.has_burr(d, 0).cpu().tolist() == [True] * 5


# ---- 6. determinism and limits --------------------------------------------------------------------------------------------
def test_same_bits_on_a_second_call_and_a_second_stream(torch_cuda, model):
    torch = torch_cuda
    r = np.random.default_rng(3)
    frames = r.integers(0, 256, (3, 2 * TH + 3, 3 * TW + 5), dtype=np.uint8)
    grey, cable = ed.make_burr_scene(96, 200, 2, noise_sigma=1.0)
    d = torch.from_numpy(frames).cuda()
    dg, dc = torch.from_numpy(grey[None]).cuda(), torch.from_numpy(cable[None]).cuda()
    run = lambda: (model.edges_combined(d), model.detect_burrs_enhanced(dg, dc), model.burr_mask_dog(dg, dc), model.has_burr(dg))
    first = run()
    assert first[0].any() and first[1].any() and first[2].any()
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(run(), first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = run()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, first))


def test_limits_raise_before_any_launch(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    small = torch.zeros((1, 7, 40), dtype=torch.uint8, device="cuda:0")
    ok = torch.zeros((1, 8, 40), dtype=torch.uint8, device="cuda:0")
    for call in (lambda: model.edges_combined(small), lambda: model.edges_combined(small, small), lambda: model.detect_burrs_enhanced(small, small),
                 lambda: model.burr_mask_dog(small, small), lambda: model.dog_band(small, small)):
        with pytest.raises(ValueError, match="8 <= H, W"):
            call()
    for taps in ([14, 62, 104, 62, 15], [128, 128], [256, 0, 0, 0, 0, 0, 0, 0, 0], [-1, 258, -1]):
        for call in (lambda t: model.burr_mask_dog(ok, ok, taps1=t), lambda t: model.dog_band(ok, ok, taps2=t),
                     lambda t: model.detect_burrs_enhanced(ok, ok, taps=t)):
            with pytest.raises(ValueError, match="taps|tap"):
                call(np.array(taps, np.int32))
    with pytest.raises(RuntimeError, match="differ in shape"):
        model.edges_combined(ok, torch.zeros((1, 8, 41), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        model.edges_combined(ok, sobel_threshold=float("nan"))
    # the C ABI refuses the same and leaves the output alone
    lib = _lib.load()
    model.canny(ok, 50, 150)                                     # makes the engine
    out = torch.full((1, 8, 40), 7, dtype=torch.uint8, device="cuda:0")
    counts = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
    assert lib.unetpp_edges_union_workspace_bytes(0) == 0 and lib.unetpp_edges_union_workspace_bytes(3) >= 12
    ws = torch.empty(int(lib.unetpp_edges_union_workspace_bytes(1)) + 16, dtype=torch.uint8, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    taps = lambda *v: (ctypes.c_int32 * len(v))(*v)
    t3, t7 = taps(70, 116, 70), taps(8, 28, 56, 72, 56, 28, 8)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = model._handle
    union, dog = lib.unetpp_edges_union_u8, lib.unetpp_dog_band_u8
    assert union(h, p(ok), p(ok), 1, 7, 40, 50, 15, p(ws), p(out), stream) == -2                 # below 8 rows
    assert union(h, p(ok), p(ok), 1, 8, 70000, 50, 15, p(ws), p(out), stream) == -2
    assert union(h, p(ok), p(ok), 0, 8, 40, 50, 15, p(ws), p(out), stream) == -1
    assert union(h, None, p(ok), 1, 8, 40, 50, 15, p(ws), p(out), stream) == -1
    assert union(h, p(ok), None, 1, 8, 40, 50, 15, p(ws), p(out), stream) == -1
    assert union(h, p(ok), p(ok), 1, 8, 40, 50, 15, None, p(out), stream) == -1
    assert union(h, p(ok), p(ok), 1, 8, 40, 50, 15, p(ws), None, stream) == -1
    assert union(h, p(ok), p(ok), 1, 8, 40, 50, 15, ctypes.c_void_p(ws.data_ptr() + 4), p(out), stream) == -1      # workspace alignment
    assert union(h, p(out), p(ok), 1, 8, 40, 50, 15, p(ws), p(out), stream) == -1                # the output over the grey image
    assert union(h, p(ok), p(out), 1, 8, 40, 50, 15, p(ws), ctypes.c_void_p(out.data_ptr() + 16), stream) == -1     # partly over the Canny image
    assert union(None, p(ok), p(ok), 1, 8, 40, 50, 15, p(ws), p(out), stream) == -1
    assert dog(h, p(ok), p(ok), 1, 7, 40, t3, 3, t7, 7, 30, p(out), stream) == -2
    assert dog(h, p(ok), p(ok), 1, 8, 40, taps(100, 100, 100), 3, t7, 7, 30, p(out), stream) == -1              # sum
    assert dog(h, p(ok), p(ok), 1, 8, 40, t3, 3, taps(128, 128), 2, 30, p(out), stream) == -1                   # even
    assert dog(h, p(ok), p(ok), 1, 8, 40, t3, 3, taps(*([28] * 8 + [32])), 9, 30, p(out), stream) == -2         # more than 7
    assert dog(h, p(ok), p(ok), 1, 8, 40, None, 3, t7, 7, 30, p(out), stream) == -1
    assert dog(h, p(ok), p(ok), 1, 8, 40, t3, 3, None, 7, 30, p(out), stream) == -1
    assert dog(h, p(ok), None, 1, 8, 40, t3, 3, t7, 7, 30, p(out), stream) == -1
    assert dog(h, p(out), p(ok), 1, 8, 40, t3, 3, t7, 7, 30, p(out), stream) == -1               # the output over an input
    assert dog(h, p(ok), p(out), 1, 8, 40, t3, 3, t7, 7, 30, p(out), stream) == -1
    assert lib.unetpp_count_nonzero_u8(h, None, 1, 8, 40, p(counts), stream) == -1
    assert lib.unetpp_count_nonzero_u8(h, p(ok), 1, 8, 40, None, stream) == -1
    assert lib.unetpp_count_nonzero_u8(h, p(ok), 1, 0, 40, p(counts), stream) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and counts.item() == 7
    # in place on the Canny image is allowed and gives the same bits
    r = np.random.default_rng(5)
    grey = torch.from_numpy(r.integers(0, 256, (2, 40, 72), dtype=np.uint8)).cuda()
    canny = model.canny(grey, 30, 100, blur=(5, 1.0))
    want = model.edges_combined(grey, canny)
    ws2 = torch.empty(int(lib.unetpp_edges_union_workspace_bytes(2)), dtype=torch.uint8, device="cuda:0")
    assert union(h, p(grey), p(canny), 2, 40, 72, 50, 15, p(ws2), p(canny), stream) == 0
    assert torch.equal(canny, want)
