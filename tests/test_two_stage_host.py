"""The two-stage loop's own steps without a GPU: the NumPy forms of unet_amd/two_stage.py against the reference's own
visualize_two_stage and map_roi_to_original (tests/golden/two_stage_scenes.npz, README_two_stage.txt), against the project's older
NumPy forms and np.rot90; the overlay table against the form it is built from on all 16 x 256 x 3 inputs; what is particular to
include/unetpp_two_stage.h (its enum, its C99 form, the null-engine codes, the guard rows the family requires); FrameStream's
argument checks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from unet_amd import _lib
from unet_amd import frame_loop
from unet_amd import robust as rb
from unet_amd import two_stage as ts
from unet_amd.simple_loops import sha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unetpp_two_stage.h")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("two_stage_scenes")
    return {k: g[k] for k in g.files}


def scenes(golden):
    for tag, h, w, seed, value, in_sha in golden["cases"]:
        frame, cable, tape, burr, roi = ts.make_scene(int(h), int(w), int(seed), int(value))
        assert sha(np.concatenate([a.reshape(-1) for a in (frame, cable, tape, burr)])) == in_sha, tag
        assert tuple(golden[tag + "_roi"].tolist()) == roi, tag
        yield tag, frame, cable, tape, burr, roi


# ---- 1. the reference's own results -------------------------------------------------------------------------------------------------
def test_overlay_np_equals_the_reference(golden):
    assert [tuple(c[:5]) for c in golden["cases"]] == [tuple(str(v) for v in s) for s in ts.FIXTURE_SCENES]
    states, values = set(), set()
    for tag, frame, cable, tape, burr, roi in scenes(golden):
        out, n_burr = ts.overlay_np(frame[None], cable[None], tape[None], burr[None], roi)
        assert out.dtype == np.uint8 and np.array_equal(out[0], golden[tag + "_out"]), tag
        assert n_burr.dtype == np.int64 and n_burr.tolist() == [int(np.count_nonzero(burr))], tag
        states |= set(np.unique(ts.overlay_states_np(frame.shape[:2], cable[None], tape[None], burr[None], roi)).tolist())
        values |= {int(m.max()) for m in (cable, tape, burr)}
        x1, y1, x2, y2 = roi
        assert 0 < x1 < x2 < frame.shape[1] and 0 < y1 < y2 < frame.shape[0], tag       # strictly inside the frame
    assert states == set(range(16)) and values == {1, 255}
    assert ts.CLASS_COLORS == {1: (0, 255, 0), 2: (255, 0, 0), 3: (255, 0, 255)} and ts.WEIGHTS == ((0.7, 0.3), (0.6, 0.4), (0.6, 0.4), (0.5, 0.5))


def test_map_roi_equals_the_reference(golden):
    for w, h, x1, y1, x2, y2 in golden["map_roi"].tolist():
        assert frame_loop.map_roi_to_original((w, h), (512, 512)) == (x1, y1, x2, y2)


def test_overlay_np_is_the_chain_of_four_blends_on_every_pixel():
    """Independent of overlay_np's array code: the four passes pixel by pixel in float32, and no pixel is left as the frame."""
    frame, cable, tape, burr, roi = ts.make_scene(9, 11, 5, 255)
    got, _ = ts.overlay_np(frame[None], cable[None], tape[None], burr[None], roi)
    f32 = np.float32
    x1, y1, x2, y2 = roi
    for y in range(9):
        for x in range(11):
            for c in range(3):
                v = frame[y, x, c]
                inside = x1 <= x < x2 and y1 <= y < y2
                v = np.uint8(np.clip(np.rint(f32(v) * f32(0.7) + f32(v if inside else 0) * f32(0.3)), 0, 255))
                for m, col, (a, b) in ((cable, (0, 255, 0), (0.6, 0.4)), (tape, (255, 0, 0), (0.6, 0.4)), (burr, (255, 0, 255), (0.5, 0.5))):
                    v = np.uint8(np.clip(np.rint(f32(v) * f32(a) + f32(col[c] if m[y, x] else 0) * f32(b)), 0, 255))
                assert got[0, y, x, c] == v, (y, x, c)
    plain = np.zeros((1, 9, 11), np.uint8)
    dimmed, n = ts.overlay_np(frame[None], plain, plain, plain, roi)
    assert (dimmed[0][frame > 8] < frame[frame > 8]).all() and n.tolist() == [0]          # 0.7 * 0.6 * 0.6 * 0.5 at best: every pixel darkens


def test_overlay_arguments():
    frame, cable, tape, burr, roi = ts.make_scene(8, 8, 0)
    colors = {1: (10, 20, 30), 2: (200, 100, 0), 3: (1, 2, 3)}
    weights = ((0.9, 0.1), (0.5, 0.5), (0.25, 0.75), (0.8, 0.3))
    a, _ = ts.overlay_np(frame[None], cable[None], tape[None], burr[None], roi, colors, weights)
    b, _ = ts.overlay_np(frame[None], cable[None], tape[None], burr[None], roi)
    assert (a != b).any()
    whole, _ = ts.overlay_np(frame[None], cable[None], tape[None], burr[None], None)
    same, _ = ts.overlay_np(frame[None], cable[None], tape[None], burr[None], (0, 0, 8, 8))
    assert np.array_equal(whole, same)
    for bad in (dict(roi=(-1, 0, 4, 4)), dict(colors={1: (0, 0, 0), 2: (0, 0, 256), 3: (0, 0, 0)}), dict(weights=((1, 0),) * 3),
                dict(weights=((float("nan"), 0),) * 4)):
        with pytest.raises(ValueError):
            ts.overlay_np(frame[None], cable[None], tape[None], burr[None], **{"roi": roi, **bad})
    with pytest.raises(ValueError, match="frames must be uint8"):
        ts.overlay_np(frame[None].astype(np.float32), cable[None], tape[None], burr[None], roi)
    with pytest.raises(ValueError, match="tape must be uint8"):
        ts.overlay_np(frame[None], cable[None], tape[None, :4], burr[None], roi)


# ---- 2. the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("custom", [False, True])
def test_overlay_table_equals_overlay_np_on_every_input(custom):
    colors = {1: (10, 250, 30), 2: (200, 100, 0), 3: (1, 2, 255)} if custom else None
    weights = ((0.9, 0.1), (0.5, 0.5), (0.25, 0.75), (0.8, 0.3)) if custom else None
    table = ts.overlay_table(colors, weights)
    assert table.shape == (16, 3, 256) and table.dtype == np.uint8 and table.flags["C_CONTIGUOUS"]
    # every (state, channel, byte) as a pixel of its own in a frame laid out differently from the one the table is built from:
    # column = state, row = byte, with a ROI of columns 8..15
    frames = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 16, axis=1).repeat(3, axis=2)[None]
    state = np.arange(16)[None, :].repeat(256, axis=0)
    masks = [(((state >> bit) & 1) * 255).astype(np.uint8)[None] for bit in (2, 1, 0)]
    want, _ = ts.overlay_np(frames, masks[0], masks[1], masks[2], (8, 0, 16, 256), colors, weights)
    assert np.array_equal(ts.overlay_states_np((256, 16), *masks, (8, 0, 16, 256))[0], state)
    for s in range(16):
        for c in range(3):
            assert np.array_equal(table[s, c], want[0, :, s, c]), (s, c)


# ---- 3. class masks, rotation, ratios --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_wh", [(53, 37), (23, 19), (48, 32), (96, 64)], ids=lambda s: "%dx%d" % s)
def test_class_masks_np_equals_the_older_resize_and_clip(size_wh, oracle):
    r = np.random.default_rng(size_wh[0])
    pred = r.integers(0, 3, (3, 32, 48), dtype=np.uint8)
    fw, fh = size_wh
    for roi in ((5, 3, fw - 4, fh - 2), (0, 0, fw, fh), None, (7, 7, 7, 12), (9, 4, 3, 12), (2, 1, fw + 10, fh + 10)):
        cable, tape, counts = ts.class_masks_np(pred, size_wh, roi)
        assert cable.dtype == tape.dtype == np.uint8 and counts.dtype == np.int64 and counts.shape == (3, 2)
        for got, c in ((cable, 1), (tape, 2)):
            for i in range(3):
                full = rb.resize_nearest_np((pred[i] == c).astype(np.uint8), size_wh)
                want = np.zeros_like(full)
                if roi is None:
                    want = full
                else:
                    x1, y1, x2, y2 = roi
                    want[y1:y2, x1:x2] = full[y1:y2, x1:x2]
                    assert np.array_equal(want, oracle.clip_to_roi_np(oracle.cv2_resize_nearest_np((pred[i] == c).astype(np.uint8), size_wh), roi))
                assert np.array_equal(got[i], want), (roi, c, i)
                assert counts[i, c - 1] == want.sum()
        if roi in ((7, 7, 7, 12), (9, 4, 3, 12)):
            assert not cable.any() and not tape.any() and not counts.any()
    with pytest.raises(ValueError, match="negative"):
        ts.class_masks_np(pred, size_wh, (-1, 0, 5, 5))
    with pytest.raises(ValueError, match="pred must be uint8"):
        ts.class_masks_np(pred.astype(np.int32), size_wh)


@pytest.mark.parametrize("shape", [(2, 37, 53, 3), (2, 37, 53, 1), (1, 1, 1, 3), (3, 16, 64, 3)], ids=str)
def test_rotate_np_equals_rot90(shape):
    x = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
    for code, name, k in ((0, "90_cw", 3), (1, "180", 2), (2, "90_ccw", 1)):      # np.rot90 turns counter-clockwise
        got = ts.rotate_np(x, code)
        assert got.flags["C_CONTIGUOUS"] and np.array_equal(got, np.rot90(x, k, axes=(1, 2)))
        assert np.array_equal(ts.rotate_np(x, name), got)
    assert np.array_equal(ts.rotate_np(ts.rotate_np(x, 0), 2), x)
    assert ts.ROTATE_CODES == {"90_cw": 0, "180": 1, "90_ccw": 2}                  # cv2.ROTATE_90_CLOCKWISE, _180, _90_COUNTERCLOCKWISE
    for bad in (3, -1, "left", True, 1.5):
        with pytest.raises(ValueError, match="code must be"):
            ts.rotate_np(x, bad)


def test_ratios():
    got = ts.ratios(np.array([[50, 25, 0], [10, 0, 3]]), 200)
    assert got[0] == {"cable_ratio": 25.0, "tape_ratio": 12.5, "burr_ratio": 0.0, "burr": False, "status": "[OK]"}
    assert got[1]["status"] == "[BURR!]" and got[1]["burr"] is True and got[1]["burr_ratio"] == 3 / 200 * 100
    assert ts.ratios([[5, 5, 5]], 0)[0] == {"cable_ratio": 0, "tape_ratio": 0, "burr_ratio": 0, "burr": True, "status": "[BURR!]"}
    assert ts.roi_area((140, 0, 270, 512)) == 130 * 512


# ---- 4. the header's entries (names, types, build inputs and guard coverage: tests/test_bindings_host.py) ---------------------------------
def test_rotate_codes_are_the_headers_enum():
    with open(HEADER) as f:
        text = f.read()
    for name, value in _lib.ROTATE_CODES.items():
        assert re.search(r"\bUNETPP_ROTATE_%s = %d\b" % (name.upper(), value), text), name


def test_header_is_c99(tmp_path):
    cc_ = shutil.which("cc") or shutil.which("gcc")
    assert cc_, "no C compiler"
    src = tmp_path / "use.c"
    src.write_text('#include "unetpp_two_stage.h"\nint main(void) { return UNETPP_ROTATE_90_CW + (UNETPP_ROTATE_180 != 1) + (UNETPP_ROTATE_90_CCW != 2); }\n')
    subprocess.run([cc_, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True, text=True)


def test_entries_refuse_a_null_engine():
    lib = _lib.load()
    assert lib.unetpp_two_stage_masks_u8(None, None, 1, 8, 8, None, None, 8, 8, 0, 0, 8, 8, None, None) == -1
    assert lib.unetpp_two_stage_overlay_u8(None, None, None, None, None, 1, 8, 8, 0, 0, 8, 8, None, None, None, None) == -1
    assert lib.unetpp_rotate_u8(None, None, 1, 8, 8, 3, 0, None, None) == -1


def test_guard_rows_the_family_requires():
    """Both frame loops have a row, and every symbol of ABI_TWO_STAGE has a row that reaches nothing else."""
    import test_gpu_guarded_two_stage as tgt
    names = [r.name for r in tgt.ROWS_TWO_STAGE]
    assert any(n.startswith("process_frames_two_stage") for n in names) and any(n.startswith("process_raw_frames_two_stage") for n in names)
    for symbol in _lib.ABI_TWO_STAGE:
        assert any(r.symbols == {symbol} for r in tgt.ROWS_TWO_STAGE), f"{symbol} has no row of its own"


def test_no_method_was_added_to_the_models():
    """Every device function of the feature is a module function that takes the model."""
    import inspect
    for fn in (ts.class_masks, ts.overlay, ts.rotate, frame_loop.process_frames_two_stage, frame_loop.process_raw_frames_two_stage):
        assert list(inspect.signature(fn).parameters)[0] == "model"
    for name in ("class_masks", "overlay", "rotate"):
        assert callable(getattr(ts, name + "_np"))


# ---- 5. FrameStream's argument checks ------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, device_index=0):
        self._device_index = device_index


def test_frame_stream_refuses_bad_arguments_before_it_touches_a_device():
    from unet_amd.stream import FrameStream
    fn = lambda m, x: x
    a = _Model()
    with pytest.raises(ValueError, match="same model was given twice"):
        FrameStream([a, a], fn)
    with pytest.raises(ValueError, match="at least one model"):
        FrameStream([], fn)
    with pytest.raises(TypeError, match="fn must be callable"):
        FrameStream([a], None)
    with pytest.raises(ValueError, match="must be on a device"):
        FrameStream([a, _Model(None)], fn)
    with pytest.raises(ValueError, match="on 2 devices"):
        FrameStream([a, _Model(1)], fn)
    for bad in ((), (1.5,), (True,), (None,)):
        with pytest.raises(ValueError, match="outputs must name"):
            FrameStream([a], fn, outputs=bad)
