"""Guard-band tests of the seventh binding table (include/unetpp_two_stage.h): every public call of unet_amd/two_stage.py and the
two-stage loop, BGR and raw, between random guard bytes, through the harness and the placements of tests/test_gpu_guarded.py, with
its four assertions: guards intact, equal to the NumPy form bit for bit, the same bits with the filling complemented, placements of
one data set bitwise equal.  The placements give ts_overlay_kernel outputs whose frames start at every phase of its 48-byte spans
(P1 aligned, P2 one byte off, P4 at 15; P3's 33 x 129 frames are 12771 bytes, so each frame of the batch has its own phase), inputs
that disagree with the output modulo 16, and a look-up table off its 16-byte boundary (the byte path of its load); ts_masks_kernel
and ts_rotate_kernel get ragged tiles in both axes (P3, P5, P6) and rows that end anywhere.
The rows live in this module's own list (ROWS_TWO_STAGE); tests/test_two_stage_host.py compares it with the table.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_two_stage.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_guarded as tg
from test_gpu_guarded import torch_cuda  # noqa: F401  (fixture)
from unet_amd import edges as ed
from unet_amd import raw_frames as rf
from unet_amd import two_stage as ts

MASKS, OVERLAY, ROTATE = ["unetpp_two_stage_masks_u8"], ["unetpp_two_stage_overlay_u8"], ["unetpp_rotate_u8"]
BURRS = ["unetpp_canny_u8", "unetpp_morphology", "unetpp_components", "unetpp_components_filter_box"]      # detect_burrs
LOOP = ["unetpp_resize_linear_u8", "unetpp_forward_ex", "unetpp_gray_u8"] + MASKS + BURRS + OVERLAY
LOOP_RAW = ["unetpp_raw_resize_u8", "unetpp_forward_ex", "unetpp_raw_to_bgr_u8"] + MASKS + BURRS + OVERLAY
NET_HW = (32, 32)
COLORS = {1: (10, 250, 30), 2: (200, 100, 0), 3: (1, 2, 255)}
WEIGHTS = ((0.9, 0.1), (0.5, 0.5), (0.25, 0.75), (0.8, 0.3))


def build_pred(s, r):
    return {"pred": tg.class_mask(s, r, 4)}


def build_overlay(s, r):
    """Frames and three masks that overlap pairwise and all at once: 8 x 8 blocks of 0 / value, the burr with 255."""
    return {"frames": tg.bgr_frames(s, r), "cable": (tg.class_mask(s, r, 2, 0.05) != 0).astype(np.uint8),
            "tape": (tg.class_mask(s, r, 2, 0.05) != 0).astype(np.uint8), "burr": ((tg.class_mask(s, r, 3, 0.05) == 1) * 255).astype(np.uint8)}


def build_gray1(s, r):
    return {"frames": tg.gray_frames(s, r)[..., None]}


def build_raw(s, r):
    return {"raw": rf.make_raw(s[0], s[1], s[2], int(r.integers(1 << 30)))}


def roi_of(a, key="frames"):
    h, w = a[key].shape[1:3]
    return (5, 3, w - 7, h - 4)


def sized(a):
    h, w = a["pred"].shape[1:]
    return (w + 21, h + 5)                                    # (width, height): a non-integer upscale


def overlay_ref(a, roi, **kw):
    return list(ts.overlay_np(a["frames"], a["cable"], a["tape"], a["burr"], roi, kw.get("colors"), kw.get("weights")))


def loop_ref(a, raw):
    """The parts' NumPy forms on the device's own pred (computed outside the guards: the network has no NumPy form here)."""
    import torch
    from unet_amd import frame_loop
    m = _net["m"]
    if raw:
        frames = rf.demosaic_np(a["raw"], "RG")
        pred = frame_loop.process_raw_frames(m, torch.from_numpy(a["raw"]).cuda(), "BayerRG8", target_size=NET_HW[::-1])[0].cpu().numpy()
    else:
        frames = a["frames"]
        pred = frame_loop.process_frames(m, torch.from_numpy(frames).cuda(), target_size=NET_HW[::-1])[0].cpu().numpy()
    roi = roi_of({"frames": frames})
    fh, fw = frames.shape[1:3]
    cable, tape, counts = ts.class_masks_np(pred, (fw, fh), roi)
    burr = np.stack([ed.detect_burrs_np(g, c) for g, c in zip(ed.bgr_to_gray_np(frames), cable)])
    over, n_burr = ts.overlay_np(frames, cable, tape, burr, roi)
    return [pred, cable, tape, burr, over, np.concatenate([counts, n_burr[:, None]], axis=1)]


def loop_call(m, t, a, raw):
    from unet_amd import frame_loop
    if raw:
        r = frame_loop.process_raw_frames_two_stage(m, t["raw"], "BayerRG8", target_size=NET_HW[::-1], roi=roi_of(a, "raw"), max_components=tg.K)
    else:
        r = frame_loop.process_frames_two_stage(m, t["frames"], target_size=NET_HW[::-1], roi=roi_of(a), max_components=tg.K)
    return [r.pred, r.mask_cable, r.mask_tape, r.mask_burr, r.result, r.counts]


_net = {}                                                     # the module's model, for loop_ref (a ref gets the arrays alone)
row = tg.Row

ROWS_TWO_STAGE = [
    row("class_masks[roi]", MASKS, build_pred, lambda m, t, a: list(ts.class_masks(m, t["pred"], sized(a), (5, 3, 120, 30))),
        lambda a: list(ts.class_masks_np(a["pred"], sized(a), (5, 3, 120, 30)))),
    row("class_masks[no roi, down]", MASKS, build_pred, lambda m, t, a: list(ts.class_masks(m, t["pred"], (19, 13))),
        lambda a: list(ts.class_masks_np(a["pred"], (19, 13)))),
    row("class_masks[empty roi]", MASKS, build_pred, lambda m, t, a: list(ts.class_masks(m, t["pred"], sized(a), (9, 4, 9, 20))),
        lambda a: list(ts.class_masks_np(a["pred"], sized(a), (9, 4, 9, 20)))),
    row("overlay[roi]", OVERLAY, build_overlay, lambda m, t, a: list(ts.overlay(m, t["frames"], t["cable"], t["tape"], t["burr"], roi_of(a))),
        lambda a: overlay_ref(a, roi_of(a))),
    row("overlay[no roi, colours and weights]", OVERLAY, build_overlay,
        lambda m, t, a: list(ts.overlay(m, t["frames"], t["cable"], t["tape"], t["burr"], None, colors=COLORS, weights=WEIGHTS)),
        lambda a: overlay_ref(a, None, colors=COLORS, weights=WEIGHTS)),
]
ROWS_TWO_STAGE += [row(f"rotate[{name}, bgr]", ROTATE, tg.B_BGR, (lambda c: lambda m, t, a: ts.rotate(m, t["frames"], c))(code),
                       (lambda c: lambda a: ts.rotate_np(a["frames"], c))(code)) for name, code in ts.ROTATE_CODES.items()]
ROWS_TWO_STAGE += [row(f"rotate[{name}, grey]", ROTATE, build_gray1, (lambda c: lambda m, t, a: ts.rotate(m, t["frames"], c))(code),
                       (lambda c: lambda a: ts.rotate_np(a["frames"], c))(code)) for name, code in ts.ROTATE_CODES.items()]
ROWS_TWO_STAGE += [
    row("process_frames_two_stage", LOOP, tg.B_BGR, lambda m, t, a: loop_call(m, t, a, False), lambda a: loop_ref(a, False)),
    row("process_raw_frames_two_stage[BayerRG8]", LOOP_RAW, build_raw, lambda m, t, a: loop_call(m, t, a, True), lambda a: loop_ref(a, True)),
]
ROW_BY_NAME = {r.name: r for r in ROWS_TWO_STAGE}


@pytest.fixture(scope="module")
def model(torch_cuda, syn):  # noqa: F811
    """The network of the loop rows (32 x 32 input, synthetic weights); every other row uses it for its launches only."""
    from unet_amd.nested_unet import NestedUNet
    m = NestedUNet(3, deep_supervision=False, max_batch=3, max_hw=NET_HW).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(3, 3, False, 2), strict=True)
    _net["m"] = m.eval()
    return _net["m"]


@pytest.mark.gpu
@pytest.mark.parametrize("placement", list(tg.PLACEMENTS))
@pytest.mark.parametrize("name", list(ROW_BY_NAME))
def test_row(torch_cuda, model, name, placement):  # noqa: F811
    r = ROW_BY_NAME[name]
    got = tg.run_row(torch_cuda, model, r, placement)
    if placement in tg.SAME_BITS:
        guarded.assert_same_bytes(tg.run_row(torch_cuda, model, r, tg.SAME_BITS[placement]), got,
                                  f"{name}: {tg.SAME_BITS[placement]} (aligned) against {placement} (the pointer says no)")
