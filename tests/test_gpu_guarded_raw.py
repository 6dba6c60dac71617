"""Guard-band tests of the sixth binding table (include/unetpp_raw.h): every public call of unet_amd/raw_frames.py and the raw
frame loop between random guard bytes, through the harness and the placements of tests/test_gpu_guarded.py, with its four
assertions: guards intact, equal to the NumPy form bit for bit, the same bits with the filling complemented, placements of one
data set bitwise equal.  The placements give rf_to_bgr_kernel one full 128 x 16 tile twice over (P1, P2, P4: aligned, one byte off,
scattered), a frame of tile + 1 in both axes (P3, 33 x 129: the last tile takes the extra column) and one below a tile (P5, P6).
The padded row keeps its padding inside the arena: the kernel must neither copy it nor let it reach a result.
The rows live in this module's own list (ROWS_RAW); tests/test_raw_frames_host.py compares it with the table.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_raw.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_guarded as tg
from test_gpu_guarded import torch_cuda  # noqa: F401  (fixture)
from unet_amd import raw_frames as rf

TO_BGR, RESIZE = ["unetpp_raw_to_bgr_u8"], ["unetpp_raw_resize_u8"]
LOOP = RESIZE + ["unetpp_forward_ex", "unetpp_resize_nearest_roi_u8"] + TO_BGR          # want_gray: the grey-only launch
NET_HW = (32, 32)


def build_raw(s, r):
    return {"raw": rf.make_raw(s[0], s[1], s[2], int(r.integers(1 << 30)))}


def build_padded(s, r):
    """Rows of w + 5 bytes: the frame is the view [:, :, :w] of it."""
    raw = rf.make_raw(s[0], s[1], s[2] + 5, int(r.integers(1 << 30)))
    return {"raw": raw, "hw": np.array(s[1:])}


def roi_of(a):
    h, w = a["raw"].shape[1:]
    return (3, 1, w - 7, h - 4)                               # an odd origin


def loop_roi(a):
    h, w = a["raw"].shape[1:]
    return (5, 2, w - 3, h - 1)                               # (x1, y1, x2, y2) in frame pixels


def loop_call(m, t, a):
    from unet_amd import frame_loop
    return list(frame_loop.process_raw_frames(m, t["raw"], "BayerRG8", target_size=NET_HW[::-1], roi=loop_roi(a), want_gray=True))


def loop_ref(a):
    """process_frames on the demosaiced frame, on the device outside the guards: the network has no NumPy form here, and
    tests/test_gpu_raw_frames.py pins to_bgr against the NumPy form."""
    import torch
    from unet_amd import frame_loop
    raw = torch.from_numpy(a["raw"]).cuda()
    bgr, gray = rf.to_bgr(_net["m"], raw, "BayerRG8", want_gray=True)
    out = frame_loop.process_frames(_net["m"], bgr, target_size=NET_HW[::-1], roi=loop_roi(a))
    return [v.cpu().numpy() for v in out + (gray,)]


_net = {}                                                     # the module's model, for loop_ref (a ref gets the arrays alone)
row = tg.Row


ROWS_RAW = [row(f"to_bgr[{p}]", TO_BGR, build_raw, (lambda p: lambda m, t, a: rf.to_bgr(m, t["raw"], pattern=p))(p),
                (lambda p: lambda a: rf.demosaic_np(a["raw"], p))(p)) for p in ("BG", "GB", "RG", "GR", "MONO")]
ROWS_RAW += [
    row("to_gray[RG]", TO_BGR, build_raw, lambda m, t, a: rf.to_gray(m, t["raw"], pattern="RG"), lambda a: rf.gray_np(a["raw"], "RG")),
    row("to_gray[BayerGR8: mono]", TO_BGR, build_raw, lambda m, t, a: rf.to_gray(m, t["raw"], "BayerGR8"), lambda a: a["raw"]),
    row("to_bgr[BayerBG8, both]", TO_BGR, build_raw, lambda m, t, a: list(rf.to_bgr(m, t["raw"], "BayerBG8", want_gray=True)),
        lambda a: [rf.demosaic_np(a["raw"], "BG"), rf.gray_np(a["raw"], "BG")]),
    row("to_bgr[GB, both, padded rows]", TO_BGR, build_padded,
        lambda m, t, a: list(rf.to_bgr(m, t["raw"][:, :, :int(a["hw"][1])], pattern="GB", want_gray=True)),
        lambda a: [rf.demosaic_np(a["raw"][:, :, :int(a["hw"][1])], "GB"), rf.gray_np(a["raw"][:, :, :int(a["hw"][1])], "GB")]),
    row("resize[RG, down]", RESIZE, build_raw, lambda m, t, a: rf.resize(m, t["raw"], "RG", (12, 40)), lambda a: rf.raw_resize_np(a["raw"], "RG", None, (12, 40))),
    row("resize[BG, up, odd roi]", RESIZE, build_raw, lambda m, t, a: rf.resize(m, t["raw"], "BG", (50, 161), roi_of(a)),
        lambda a: rf.raw_resize_np(a["raw"], "BG", roi_of(a), (50, 161))),
    row("resize[GR, padded rows, odd roi]", RESIZE, build_padded, lambda m, t, a: rf.resize(m, t["raw"][:, :, :int(a["hw"][1])], "GR", (9, 33), (1, 1, 15, 13)),
        lambda a: rf.raw_resize_np(a["raw"][:, :, :int(a["hw"][1])], "GR", (1, 1, 15, 13), (9, 33))),
    row("resize[MONO]", RESIZE, build_raw, lambda m, t, a: rf.resize(m, t["raw"], "MONO", (16, 16)), lambda a: rf.raw_resize_np(a["raw"], "MONO", None, (16, 16))),
    row("process_raw_frames[BayerRG8]", LOOP, build_raw, loop_call, loop_ref),
]
ROW_BY_NAME = {r.name: r for r in ROWS_RAW}


@pytest.fixture(scope="module")
def model(torch_cuda, syn):  # noqa: F811
    """The network of the loop row (32 x 32 input, synthetic weights); every other row uses it for its launches only."""
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
