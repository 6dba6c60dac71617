"""Guard-band tests of the second binding table (include/unetpp_roi.h): every public call of unet_amd/roi_loop.py between
random guard bytes, through the harness and the placements of tests/test_gpu_guarded.py, with its four assertions: guards
intact, equal to the NumPy form bit for bit, the same bits with the filling complemented, placements of one data set bitwise
equal.  The rows live in this module's own list (ROWS_ROI): tests/test_guarded_host.py compares test_gpu_guarded.ROWS with
the first table, tests/test_roi_loop_host.py compares ROWS_ROI with the second.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_roi.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_guarded as tg
from test_gpu_guarded import model, torch_cuda  # noqa: F401  (fixtures)
from unet_amd import edges as ed
from unet_amd import roi_loop as rl

K = tg.K
# Symbols of the second table that write no caller-provided device buffer.  run_row subtracts the first table's exclusions
# only, so a row names the size query its wrapper calls beside the launching entry.
EXCLUDED_ROI = {"unetpp_roi_projection_workspace_bytes": "size query", "unetpp_roi_stats_workspace_bytes": "size query"}
PROJ, STATS = "unetpp_roi_projection_workspace_bytes", "unetpp_roi_stats_workspace_bytes"
GEOMETRY = dict(min_area=20, min_aspect=1.0, wide_width=10, edge_lo=0.1, edge_hi=0.9, large_area=150)      # scaled to 32 x 128
PRIMARY = dict(min_area=20, min_aspect=0.5)
FRAME = (47, 150)                                                          # what paste_masks pastes into
SIZE = (24, 40)                                                            # what crop_resize resizes to


def roi_table(B, W):
    """A table with a proper range, an empty one (valid = 0), the whole frame, then narrow ranges."""
    rows = [(W // 5, W - W // 4, 1, 1), (3, 3, 1, 0), (0, W, 0, 1), (W // 2, W // 2 + 1, 1, 1)]
    return np.int32([rows[b % len(rows)] for b in range(B)])


def build_edges(s, r):
    e = tg.per_frame(lambda g: ed.canny_np(g, 50, 150), tg.gray_frames(s, r))
    e[-1] = 0                                                              # no edge: the fallback
    return {"edges": e}


def build_probs(C):
    def build(s, r):
        p = tg.prob_planes((s[0], C, s[1], s[2]), r)
        thr = np.float32([[0.5, 0.55, 0.2], [0.8, 0.3, 0.35], [0.1, 0.1, 0.05]])
        return {"probs": p, "thresholds": np.ascontiguousarray(thr[np.arange(s[0]) % 3])}
    return build


def ref_thresholds(a):
    out = [rl.adaptive_thresholds_np(p) for p in a["probs"]]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def ref_ultra(a):
    out = [rl.ultra_strict_np(p, t) for p, t in zip(a["probs"], a["thresholds"])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def ref_paste(a):
    return tuple(np.stack([rl.paste_mask_np(m, q, FRAME) for m, q in zip(a[k], a["roi"])]) for k in ("mask", "other"))


ROWS_ROI = [
    tg.Row("roi_from_edges", ["unetpp_roi_from_edges_u8", PROJ], build_edges, lambda m, t, a: rl.roi_from_edges(m, t["edges"]),
           lambda a: tg.per_frame(rl.roi_from_edges_np, a["edges"])),
    tg.Row("detect_roi", ["unetpp_gray_u8", "unetpp_canny_u8", "unetpp_roi_from_edges_u8", PROJ], tg.B_BGR,
           lambda m, t, a: rl.detect_roi(m, t["frames"]), lambda a: tg.per_frame(rl.detect_roi_np, a["frames"])),
    tg.Row("crop_resize", ["unetpp_roi_crop_resize_u8"], lambda s, r: {"frames": tg.bgr_frames(s, r), "roi": roi_table(s[0], s[2])},
           lambda m, t, a: rl.crop_resize(m, t["frames"], t["roi"], SIZE),
           lambda a: tg.per_frame(lambda f, q: rl.crop_resize_np(f, q, SIZE), a["frames"], a["roi"])),
    tg.Row("adaptive_thresholds", ["unetpp_roi_adaptive_thresholds_f32", STATS], build_probs(3),
           lambda m, t, a: rl.adaptive_thresholds(m, t["probs"]), ref_thresholds),
    tg.Row("adaptive_thresholds[4 classes]", ["unetpp_roi_adaptive_thresholds_f32", STATS], build_probs(4),
           lambda m, t, a: rl.adaptive_thresholds(m, t["probs"]), ref_thresholds),
    tg.Row("ultra_strict", ["unetpp_roi_ultra_strict_f32"], build_probs(3), lambda m, t, a: rl.ultra_strict(m, t["probs"], t["thresholds"]), ref_ultra),
    tg.Row("ultra_strict[4 classes]", ["unetpp_roi_ultra_strict_f32"], build_probs(4), lambda m, t, a: rl.ultra_strict(m, t["probs"], t["thresholds"]),
           ref_ultra),
    tg.Row("refine_by_geometry", ["unetpp_components", "unetpp_roi_components_select"], tg.B_MASK,
           lambda m, t, a: rl.refine_by_geometry(m, t["mask"], match_class=1, out_value=7, max_components=K, **GEOMETRY),
           lambda a: tg.per_frame(lambda f: rl.refine_by_geometry_np(f == 1, out_value=7, **GEOMETRY), a["mask"])),
    tg.Row("select_primary", ["unetpp_components", "unetpp_roi_components_select"], tg.B_MASK,
           lambda m, t, a: rl.select_primary(m, t["mask"], match_class=2, out_value=9, max_components=K, **PRIMARY),
           lambda a: tg.per_frame(lambda f: rl.select_primary_np(f == 2, out_value=9, **PRIMARY), a["mask"])),
    tg.Row("paste_masks", ["unetpp_roi_paste_masks_u8"],
           lambda s, r: {"mask": (tg.class_mask(s, r) == 1).astype(np.uint8), "other": (tg.class_mask(s, r) == 2).astype(np.uint8),
                         "roi": roi_table(s[0], FRAME[1])},
           lambda m, t, a: rl.paste_masks(m, (t["mask"], t["other"]), t["roi"], FRAME), ref_paste),
]
ROW_BY_NAME = {r.name: r for r in ROWS_ROI}


@pytest.mark.gpu
@pytest.mark.parametrize("placement", list(tg.PLACEMENTS))
@pytest.mark.parametrize("name", list(ROW_BY_NAME))
def test_row(torch_cuda, model, name, placement):  # noqa: F811
    r = ROW_BY_NAME[name]
    got = tg.run_row(torch_cuda, model, r, placement)
    if placement in tg.SAME_BITS:
        guarded.assert_same_bytes(tg.run_row(torch_cuda, model, r, tg.SAME_BITS[placement]), got,
                                  f"{name}: {tg.SAME_BITS[placement]} (aligned) against {placement} (the pointer says no)")
