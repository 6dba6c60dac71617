"""Binary morphology programs on the device (unetpp_morphology) against the NumPy restatement
(unet_amd/morphology.py) and the fixtures made from the reference's own functions (tests/golden/morph_scenes.npz).
Everything is boolean: exact equality, no tolerance.
Run on the GPU box:  python -m pytest tests/test_gpu_morphology.py -m gpu"""
import ctypes
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import components as cc
from unet_amd import morphology as mo

pytestmark = pytest.mark.gpu

OPS4 = ("dilate", "erode", "open", "close")
ELEMENTS = [("ellipse", 2), ("ellipse", 3), ("ellipse", 5), ("ellipse", 8), ("ellipse", 15), ("ellipse", 21), ("ellipse", 25),
            ("ellipse", 63), ("rect", (1, 9)), ("rect", (9, 1)), ("cross", 7)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def model(torch_cuda):
    from unet_amd.nested_unet import NestedUNet
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: morphology needs none


def single_np(masks, match_class, op, element, anchor=None, iterations=1, out_value=1):
    el, steps, res = mo.program_single(op, element, anchor, iterations)
    return mo.run_program_np(masks, None, el, steps, match_class, -1, res, out_value)


def layout(B, H, W, element, steps, anchor=(-1, -1)):
    """(band rows, tile columns) of the kernel for a one-element program, from the library."""
    from unet_amd import _lib
    lib = _lib.load()
    e = np.ascontiguousarray(element, np.uint8)
    el = (_lib.MorphElement * 1)(_lib.MorphElement(e.shape[1], e.shape[0], anchor[0], anchor[1], e.ctypes.data))
    st = (_lib.MorphStep * len(steps))(*[_lib.MorphStep(*s) for s in steps])
    band, cols = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.unetpp_morphology_layout(B, H, W, el, 1, st, len(steps), ctypes.byref(band), ctypes.byref(cols)) == 0
    return band.value, cols.value


def random_masks(hw, seed, n=3):
    r = np.random.default_rng(seed)
    dens = (0.02, 0.5, 0.97)
    return np.stack([(r.random(hw) < dens[i % 3]).astype(np.uint8) * np.uint8(1 + i % 2) for i in range(n)])


# ---- 1. the fixtures from the reference's own functions ----------------------------------------------------------------
def fixture_cases():
    g = load_golden("morph_scenes")
    by_kind = {}
    for tag, kind, H, W, seed, param, sha in (tuple(r) for r in g["cases"].tolist()):
        by_kind.setdefault((kind, int(H), int(W), int(param)), []).append((tag, int(seed), sha))
    return g, by_kind


def test_fixture_cases_through_the_public_methods(torch_cuda, model):
    torch = torch_cuda
    g, by_kind = fixture_cases()
    seen = 0
    for (kind, H, W, param), cases in by_kind.items():
        gen = (lambda s: mo.make_hole_scene(H, W, s, noise=0.0 if H < 100 else 0.02)) if kind == "holes" else (lambda s: cc.make_scene_mask(H, W, s))
        masks = [gen(seed) for _, seed, _ in cases]
        for m, (_, _, sha) in zip(masks, cases):
            assert hashlib.sha256(m.tobytes()).hexdigest() == sha
        unpack = lambda tag, name: np.unpackbits(g[f"{tag}_{name}"])[:H * W].reshape(H, W)
        # once each frame alone (B = 1), once the group twice over in one call (B = 4 for the scene pairs)
        for batch in [[i] for i in range(len(cases))] + [list(range(len(cases))) * 2]:
            d = torch.from_numpy(np.stack([masks[i] for i in batch])).cuda()
            tags = [cases[i][0] for i in batch]
            if kind == "ring_raw":
                got = model.constrain_tape_to_ring(d, d, 2, 1).cpu().numpy()
                ref = np.stack([unpack(t, "out") for t in tags]) * np.uint8(255)
            elif kind == "ring_largest":
                cable = model.filter_components(d, 1, rule="largest", min_area=50)
                got = model.constrain_tape_to_ring(d, cable, 2, -1).cpu().numpy()
                ref = np.stack([unpack(t, "out") for t in tags]) * np.uint8(255)
            elif kind == "cleanup":
                got = model.morphology_cleanup(d, 2, param, out_value=255).cpu().numpy()
                ref = np.stack([unpack(t, "out") for t in tags]) * np.uint8(255)
            elif kind == "postprocess":
                cable, tape = model.postprocess_masks(d, 1, 2, W)
                got = np.stack([cable.cpu().numpy(), tape.cpu().numpy()])
                ref = np.stack([np.stack([unpack(t, "cable") for t in tags]), np.stack([unpack(t, "tape") for t in tags])]) * np.uint8(255)
            else:
                n, area = model.tape_holes(d, 2, hole_min_size=param)
                assert n.dtype == torch.int64 and area.dtype == torch.int64 and n.is_cuda
                assert n.tolist() == [int(g[t + "_num_holes"]) for t in tags]
                assert area.tolist() == [int(g[t + "_hole_area"]) for t in tags]
                el, steps, res = mo.program_holes()
                got = model.morphology_program(d, 2, steps, el, result_plane=res).cpu().numpy()
                ref = np.stack([unpack(t, "holes") for t in tags])
            assert got.dtype == np.uint8 and np.array_equal(got, ref), (kind, H, W, param, batch)
            seen += len(batch)
    assert seen == 26 * 3


# ---- 2. every op, element and size against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("hw", [(512, 512), (448, 800), (1024, 1024), (37, 53), (1, 200), (200, 1), (64, 64), (65, 129), (40, 2500),
                                (130, 4096)])
def test_ops_elements_and_sizes_match_restatement(hw, torch_cuda, model):
    torch = torch_cuda
    big = hw[0] * hw[1] > 600000
    masks = random_masks(hw, hw[0] * 7919 + hw[1], 2 if big else 3)
    d = torch.from_numpy(masks).cuda()
    for shape, k in ELEMENTS:
        e = mo.structuring_element(shape, k)
        for op in OPS4:
            got = model.morphology(d, -1, op, k, shape).cpu().numpy()
            assert np.array_equal(got, single_np(masks, -1, op, e)), (hw, shape, k, op)
    # a caller-supplied element gives what the named one gives
    e8 = mo.structuring_element("ellipse", 8)
    assert torch.equal(model.morphology(d, -1, "close", element=e8), model.morphology(d, -1, "close", 8))


@pytest.mark.parametrize("hw", [(512, 512), (65, 129), (37, 53)])
def test_iterations_anchor_class_and_out_value(hw, torch_cuda, model):
    torch = torch_cuda
    r = np.random.default_rng(hw[1])
    masks = r.integers(0, 3, (3,) + hw, dtype=np.uint8) * (r.random((3,) + hw) < 0.4)
    masks = np.ascontiguousarray(masks.astype(np.uint8))
    d = torch.from_numpy(masks).cuda()
    custom = np.array([[0, 1, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 1, 0]], np.uint8)
    for match_class in (-1, 1, 2):
        for out_value in (1, 255):
            for it in (1, 2, 3):
                for op in OPS4:
                    for shape, k in (("ellipse", 5), ("cross", 7)):
                        got = model.morphology(d, match_class, op, k, shape, iterations=it, out_value=out_value).cpu().numpy()
                        ref = single_np(masks, match_class, op, mo.structuring_element(shape, k), None, it, out_value)
                        assert np.array_equal(got, ref), (hw, match_class, out_value, it, op, shape)
            for op in OPS4:
                for e, anchor in ((custom, (4, 0)), (custom, (0, 2)), (mo.structuring_element("rect", (9, 1)), (7, 0)),
                                  (mo.structuring_element("ellipse", 8), (0, 7))):
                    got = model.morphology(d, match_class, op, element=e, anchor=anchor, iterations=2, out_value=out_value).cpu().numpy()
                    assert np.array_equal(got, single_np(masks, match_class, op, e, anchor, 2, out_value)), (hw, op, anchor)


# ---- 3. aimed at the band / border handling ----------------------------------------------------------------------------
def test_constant_frames_and_frames_touching_every_edge(torch_cuda, model):
    torch = torch_cuda
    for hw in ((512, 512), (130, 4096), (37, 53)):
        ones, zeros = np.ones((1,) + hw, np.uint8), np.zeros((1,) + hw, np.uint8)
        for shape, k in (("ellipse", 15), ("ellipse", 25), ("ellipse", 63), ("ellipse", 8)):
            for op in OPS4:
                for it in (1, 2):
                    if it * 2 * (k - 1) > mo.MAX_REACH and op in ("open", "close"):
                        continue
                    assert int(model.morphology(torch.from_numpy(ones).cuda(), 1, op, k, shape, iterations=it).min()) == 1, (hw, k, op)
                    assert int(model.morphology(torch.from_numpy(zeros).cuda(), 1, op, k, shape, iterations=it).max()) == 0, (hw, k, op)
    H, W = 512, 512
    y = np.arange(H)[:, None]; x = np.arange(W)[None, :]
    frame = ((np.abs(x - W / 2) < 90) | (np.abs(y - H / 2) < 40) | ((x < 9) & (y < 300)) | ((y > H - 6) & (x > 100))).astype(np.uint8)
    frame[200:230, 240:250] = 0
    assert frame[0].any() and frame[-1].any() and frame[:, 0].any() and frame[:, -1].any()
    d = torch.from_numpy(frame[None]).cuda()
    eroded = model.morphology(d, 1, "erode", 15).cpu().numpy()
    assert np.array_equal(eroded, single_np(frame[None], 1, "erode", mo.structuring_element("ellipse", 15)))
    assert eroded[0, 0].any() and eroded[0, :, -1].any()                       # not eroded from the frame's edges
    closed = model.morphology(d, 1, "close", 25).cpu().numpy()
    assert np.array_equal(closed, single_np(frame[None], 1, "close", mo.structuring_element("ellipse", 25)))
    assert closed[0, 215, 245] == 1


@pytest.mark.parametrize("hw,k", [((512, 512), 5), ((512, 512), 25), ((300, 4096), 63), ((130, 2500), 15)])
def test_single_pixels_around_every_band_and_tile_boundary(hw, k, torch_cuda, model):
    torch = torch_cuda
    H, W = hw
    e = mo.structuring_element("ellipse", k)
    close = [(0, 2, 0, 0, 0, 1), (1, 2, 2, 0, 0, 1)]
    band, cols = layout(1, H, W, e, close)
    ys = sorted({0, H - 1} | {v for b in range(band, H, band) for v in (b - 1, b)})
    xs = sorted({0, W - 1, 63, 64} | {v for c in range(cols, W, cols) for v in (c - 1, c)})
    frames = []
    for i, yy in enumerate(ys):                     # one pixel per boundary row, walking through the boundary columns
        f = np.zeros((H, W), np.uint8)
        f[yy, xs[i % len(xs)]] = 1
        frames.append(f)
    allpx = np.zeros((H, W), np.uint8)
    allpx[np.ix_(ys, xs)] = 1
    frames += [allpx, 1 - allpx]                    # every boundary pixel at once, and the same as holes
    for lo in range(0, len(frames), 8):
        masks = np.stack(frames[lo:lo + 8])
        d = torch.from_numpy(masks).cuda()
        assert layout(len(masks), H, W, e, close) == (band, cols)               # same tiles as the ones aimed at
        for op in OPS4:
            got = model.morphology(d, 1, op, k).cpu().numpy()
            assert np.array_equal(got, single_np(masks, 1, op, e)), (hw, k, op, lo)


def test_adversarial_masks_and_speckled_net_masks(torch_cuda, model):
    torch = torch_cuda
    e5 = mo.structuring_element("ellipse", 5)
    band, cols = layout(8, 512, 512, e5, [(0, 2, 0, 0, 0, 1), (1, 2, 2, 0, 0, 1)])
    adv = cc.make_adversarial_masks(512, 512, tile_h=band, tile_w=min(cols, 512))
    masks = np.stack(list(adv.values()))
    assert len(masks) == 8
    d = torch.from_numpy(masks).cuda()
    for op in ("close", "open"):
        assert np.array_equal(model.morphology(d, 1, op, 5).cpu().numpy(), single_np(masks, 1, op, e5)), op
    net = np.ascontiguousarray(load_golden("b_c3_512x512_b16")["mask"])
    assert net.shape == (16, 512, 512)
    dn = torch.from_numpy(net).cuda()
    el, steps, res = mo.program_ring()
    got = model.morphology_program(dn, 2, steps, el, mask1=dn, match1=1, result_plane=res, out_value=255).cpu().numpy()
    ref = mo.run_program_np(net, net, el, steps, 2, 1, res, 255)
    assert np.array_equal(got, ref) and ref.any()
    ring = model.constrain_tape_to_ring(dn, dn, 2, 1).cpu().numpy()
    assert np.array_equal(ring, np.stack([mo.constrain_tape_to_ring_np(m, m, 2, 1) for m in net]))
    band_ref = np.stack([mo.run_program_np(m, None, *mo.program_band(10)[:2], 1, -1, 2, 255) for m in net[:4]])
    assert np.array_equal(model.boundary_band(dn[:4], 1, band_out=10).cpu().numpy(), band_ref) and band_ref.any()


# ---- 4. programs ---------------------------------------------------------------------------------------------------------
def test_two_mask_program_and_a_full_program(torch_cuda, model):
    torch = torch_cuda
    a = np.stack([cc.make_scene_mask(448, 800, s) for s in range(3)])
    b = np.stack([cc.make_scene_mask(448, 800, 10 + s) for s in range(3)])
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    el = [mo.structuring_element("ellipse", 15), (mo.structuring_element("ellipse", 8), (2, 6)), mo.structuring_element("cross", 3),
          mo.structuring_element("rect", (9, 1))]
    two = [("dilate", 2, 0, 0, 0, 1), ("erode", 3, 1, 0, 1, 1), ("andnot", 2, 2, 3)]
    got = model.morphology_program(da, 2, two, el, mask1=db, match1=1, result_plane=2, out_value=9).cpu().numpy()
    ref = mo.run_program_np(a, b, el, two, 2, 1, 2, 9)
    assert np.array_equal(got, ref) and ref.any()
    swapped = model.morphology_program(db, 1, two, el, mask1=da, match1=2, result_plane=2, out_value=9).cpu().numpy()
    assert np.array_equal(swapped, mo.run_program_np(b, a, el, two, 1, 2, 2, 9)) and not np.array_equal(swapped, got)
    full = [("dilate", 2, 0, 0, 0, 1), ("erode", 3, 1, 0, 1, 2), ("or", 0, 2, 3), ("dilate", 1, 1, 0, 2, 3), ("andnot", 3, 0, 1),
            ("erode", 3, 3, 0, 3, 1), ("copy", 2, 3), ("and", 2, 2, 0)]
    for result_plane in (0, 1, 2, 3):
        got = model.morphology_program(da, -1, full, el, mask1=db, match1=2, result_plane=result_plane).cpu().numpy()
        assert np.array_equal(got, mo.run_program_np(a, b, el, full, -1, 2, result_plane, 1)), result_plane
    # a program of pointwise steps only, and no steps at all: the foreground itself
    assert np.array_equal(model.morphology_program(da, 1, [], [], result_plane=0).cpu().numpy(), (a == 1).astype(np.uint8))
    assert np.array_equal(model.morphology_program(da, 1, [("or", 3, 0, 1)], [], mask1=db, match1=1, result_plane=3).cpu().numpy(),
                          ((a == 1) | (b == 1)).astype(np.uint8))


# ---- 5. end to end on the network's own output -----------------------------------------------------------------------------
def test_postprocess_end_to_end_on_segment_output(torch_cuda, syn):
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    g = load_golden("b_c3_512x512")
    kinds = [str(k) for k in g["kinds"]]
    frames = np.stack([syn.make_frame_u8(512, 512, i, kinds[i % len(kinds)], int(g["fseed"])) for i in range(int(g["B"]))])
    net = NestedUNet(3, deep_supervision=True, max_batch=2, max_hw=(512, 512)).to("cuda:0")
    net.load_state_dict(syn.make_state_dict(3, 3, True, int(g["wseed"])), strict=True)
    x = torch.from_numpy(syn.frames_to_chw_f32(frames)).cuda()
    pred = net.eval().segment(x)
    before = pred.clone()
    host = pred.cpu().numpy()
    n, area = net.tape_holes(pred, 2, hole_min_size=3)
    ref = [mo.tape_holes_np(m, 2, 3) for m in host]
    assert n.tolist() == [r[0] for r in ref] and area.tolist() == [r[1] for r in ref] and sum(r[0] for r in ref) > 0
    ring = net.constrain_tape_to_ring(pred, pred, 2, 1)
    assert np.array_equal(ring.cpu().numpy(), np.stack([mo.constrain_tape_to_ring_np(m, m, 2, 1) for m in host]))
    assert int(ring.count_nonzero()) > 0
    for kw in ({}, {"min_area": 50, "min_aspect": 1.0, "max_center_offset": 0.5}):
        cable, tape = net.postprocess_masks(pred, 1, 2, 512, **kw)
        refs = [mo.postprocess_masks_np(m, 1, 2, 512, **kw) for m in host]
        assert np.array_equal(cable.cpu().numpy(), np.stack([r[0] for r in refs]))
        assert np.array_equal(tape.cpu().numpy(), np.stack([r[1] for r in refs]))
    assert any(r[1].any() for r in refs)                              # the looser gates keep a cable, so a ring exists
    assert net.status() == 0 and torch.equal(net.segment(x), before) and torch.equal(pred, before)


def test_simple_unet_inherits_the_methods(torch_cuda):
    torch = torch_cuda
    from unet_amd.nested_unet import SimpleUNet
    m = SimpleUNet(3).to("cuda:0")
    mask = cc.make_scene_mask(64, 96, 3, noise=0.1)[None]
    got = m.morphology_cleanup(torch.from_numpy(mask).cuda(), 2, 3)
    assert np.array_equal(got[0].cpu().numpy(), mo.cleanup_np(mask[0], 2, 3))


# ---- 6. the C ABI's error returns -----------------------------------------------------------------------------------------
def test_c_abi_error_returns_leave_the_output_untouched(torch_cuda, model):
    torch = torch_cuda
    from unet_amd import _lib
    lib = _lib.load()
    B, H, W = 2, 40, 72
    model.morphology(torch.zeros((B, H, W), dtype=torch.uint8, device="cuda"))       # makes sure the engine exists
    h = model._handle
    buf = torch.zeros((3 * B * H * W,), dtype=torch.uint8, device="cuda")
    mask, out = buf[:B * H * W], buf[2 * B * H * W:]
    mask[::3] = 1
    out.fill_(77)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    err = lambda: lib.unetpp_last_error(h).decode()
    e5 = mo.structuring_element("ellipse", 5)

    def run(element=e5, steps=((0, 2, 0, 0, 0, 1), (1, 2, 2, 0, 0, 1)), result=2, mask0=mask, mask1=None, out_=out, anchor=(-1, -1),
            n_elements=1, hh=H, match0=-1):
        e = np.ascontiguousarray(element, np.uint8)
        el = (_lib.MorphElement * 1)(_lib.MorphElement(e.shape[1], e.shape[0], anchor[0], anchor[1], e.ctypes.data))
        st = (_lib.MorphStep * max(len(steps), 1))(*[_lib.MorphStep(*s) for s in steps])
        return lib.unetpp_morphology(h, p(mask0), match0, p(mask1), -1, B, hh, W, el, n_elements, st, len(steps), result, 255, p(out_), None)

    inv, uns = -1, -2
    assert run(steps=((6, 2, 0, 0, 0, 1),)) == inv and "op" in err()
    assert run(steps=((0, 4, 0, 0, 0, 1),)) == inv and "plane" in err()
    assert run(steps=((0, 2, 0, 0, 1, 1),)) == inv and "element index" in err()
    assert run(steps=((2, 2, 0, 3, 0, 1),)) == inv and "before any step has written it" in err()
    assert run(result=3) == inv and "result_plane" in err()
    assert run(steps=((0, 2, 0, 0, 0, 0),)) == inv and "iterations" in err()
    assert run(element=np.ones((3, 64), np.uint8)) == uns and "too large" in err()
    assert run(element=np.array([[1, 0, 1]], np.uint8)) == uns and "row-convex" in err()
    assert run(element=np.zeros((3, 3), np.uint8)) == inv and "empty" in err()
    assert run(anchor=(0, 5)) == inv and "anchor" in err()
    assert run(element=mo.structuring_element("ellipse", 63), steps=((0, 2, 0, 0, 0, 1), (1, 2, 2, 0, 0, 1), (0, 2, 2, 0, 0, 1))) == uns and "reach" in err()
    assert run(steps=((0, 2, 0, 0, 0, 1),) * 9) == inv and "n_steps" in err()
    assert run(n_elements=5) == inv and "n_elements" in err()
    assert run(hh=0) == inv and "shape" in err()
    assert run(match0=256) == inv and "match_class" in err()
    assert run(mask0=None) == inv and run(out_=None) == inv and "null" in err()
    assert run(out_=mask) == inv and "aliases" in err()
    assert run(mask1=out) == inv and "aliases" in err()
    assert run(out_=buf[B * H * W - 16:2 * B * H * W - 16]) == inv and "aliases" in err()      # a partial overlap
    assert lib.unetpp_morphology(None, p(mask), -1, None, -1, B, H, W, None, 0, None, 0, 0, 1, p(out), None) == inv
    torch.cuda.synchronize()
    assert int((out != 77).sum()) == 0                                      # no failed call wrote anything
    assert run() == 0
    torch.cuda.synchronize()
    host = mask.cpu().numpy().reshape(B, H, W)
    assert np.array_equal(out.cpu().numpy().reshape(B, H, W), single_np(host, -1, "close", e5, out_value=255))
    with pytest.raises(ValueError, match="reach"):                          # the method's own check, before any device call
        model.morphology(mask.reshape(B, H, W), ksize=63, op="close", iterations=2)


# ---- 7. reproducible bit for bit --------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_and_on_a_second_stream(torch_cuda, model):
    torch = torch_cuda
    masks = np.stack([cc.make_scene_mask(512, 512, s) for s in range(4)])
    d = torch.from_numpy(masks).cuda()
    calls = [lambda: model.morphology(d, 2, "close", 25), lambda: model.constrain_tape_to_ring(d, d, 2, 1), lambda: model.morphology_cleanup(d, 2, 5)]
    first = [c() for c in calls]
    second = [c() for c in calls]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = [c() for c in calls]
    side.synchronize()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c) and int(a.count_nonzero()) > 0


# ---- 8. nothing else moved --------------------------------------------------------------------------------------------------
def test_segment_components_and_filters_are_what_they_were(torch_cuda, syn, model):
    torch = torch_cuda
    from unet_amd.nested_unet import NestedUNet
    g = load_golden("s_c3_128x96")
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    net = NestedUNet(3, deep_supervision=True, max_batch=B, max_hw=(H, W)).to("cuda:0")
    net.load_state_dict(syn.make_state_dict(3, 3, True, int(g["wseed"])), strict=True)
    frames = syn.make_frames_u8(B, H, W, str(g["kind"]), int(g["fseed"]))
    mask = net.eval().segment(torch.from_numpy(frames).cuda())
    net.morphology(mask, 1, "close", 5)                                   # a morphology call in between changes nothing
    assert np.array_equal(mask.cpu().numpy(), g["mask"])
    assert np.array_equal(net.segment(torch.from_numpy(frames).cuda()).cpu().numpy(), g["mask"])
    gc = load_golden("cc_scenes")
    tag, H, W, seed, cls, sha = next(tuple(r) for r in gc["cases"].tolist())
    H, W, seed, cls = int(H), int(W), int(seed), int(cls)
    scene = cc.make_scene_mask(H, W, seed)
    assert hashlib.sha256(scene.tobytes()).hexdigest() == sha
    d = torch.from_numpy(scene[None]).cuda()
    labels, num, stats, cen = model.components(d, cls)
    assert int(num[0]) == int(gc[tag + "_num"]) and np.array_equal(stats[0, :64].cpu().numpy(), gc[tag + "_stats"])
    assert np.array_equal(cen[0, 1:64].cpu().numpy(), gc[tag + "_centroids"][1:64])
    for rule, kw, out_value in (("largest", {"min_area": 50}, 1), ("cable_shape", {}, 255), ("spatial", {}, 1)):
        got = model.filter_components(d, cls, rule=rule, out_value=out_value, **kw)[0].cpu().numpy()
        assert np.array_equal(got, np.unpackbits(gc[f"{tag}_{rule}"])[:H * W].reshape(H, W) * np.uint8(out_value)), rule
