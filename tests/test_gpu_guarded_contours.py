"""Guard-band tests of the fourth binding table (include/unetpp_contours.h): every public call of unet_amd/contours.py between
random guard bytes, through the harness and the placements of tests/test_gpu_guarded.py, with its four assertions: guards
intact, equal to the NumPy form bit for bit, the same bits with the filling complemented, placements of one data set bitwise
equal.  The rows live in this module's own list (ROWS_CONTOURS); tests/test_contours.py compares it with the fourth table.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_contours.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_guarded as tg
from test_gpu_guarded import model, torch_cuda  # noqa: F401  (fixtures)
from unet_amd import contours as ct

# Symbols of the fourth table that write no caller-provided device buffer.  The size query is still listed by the rows that
# make it: the harness empties the workspace cache, so every run asks again.
EXCLUDED_CONTOURS = {"unetpp_contours_workspace_bytes": "size query"}
K = 512
AREAS = ["unetpp_contour_areas_u8", "unetpp_contours_workspace_bytes"]
CIRCLE = AREAS + ["unetpp_contour_circle"]


def per_frame(fn, a):
    return np.stack([np.asarray(fn(f)) for f in a])


def ref_areas(a, match):
    labels, nums, areas = [], [], []
    for f in a["mask"]:
        l, n, ar = ct.external_contour_areas_np(f, match)
        labels.append(l); nums.append(n); areas.append(np.concatenate([ar, np.zeros(K - n, np.int64)]))
    return [np.stack(labels), np.array(nums, np.int32), np.stack(areas)]


def call_circle(m, t, match):
    table = ct.enclosing_circle(m, t["mask"], match, K)
    return [table[:, 7], np.array([(c[0][0], c[0][1], c[1]) for c in ct.circle_from_support(table.cpu().numpy())])]


def ref_circle(a, match):
    got = [ct.support_table_np(f, match) for f in a["mask"]]
    return [np.array([g[0] for g in got], np.int32), np.array([(g[1][0][0], g[1][0][1], g[1][1]) for g in got])]


def build_overlay(s, r):
    return {"frames": tg.bgr_frames(s, r), "cable": (tg.class_mask(s, r) == 1).astype(np.uint8) * 255, "tape": (tg.class_mask(s, r) == 2).astype(np.uint8) * 255,
            "burr": (r.random(s) < 0.1).astype(np.uint8)}


def paste_row(name, roi_of, frame_of):
    return tg.Row(name, ["unetpp_paste_roi_u8"], tg.B_MASK, lambda m, t, a: ct.paste_roi_masks(m, t["mask"], roi_of(a["mask"].shape), frame_of(a["mask"].shape)),
                  lambda a: ct.paste_roi_masks_np(a["mask"], roi_of(a["mask"].shape), frame_of(a["mask"].shape)))


ROWS_CONTOURS = [
    tg.Row("outer_border[class 1]", AREAS, tg.B_MASK, lambda m, t, a: ct.outer_border(m, t["mask"], 1, K),
           lambda a: per_frame(lambda f: ct.outer_border_np(f, 1), a["mask"])),
    tg.Row("external_contour_areas[class 2]", AREAS, tg.B_MASK, lambda m, t, a: list(ct.external_contour_areas(m, t["mask"], 2, K)), lambda a: ref_areas(a, 2)),
    tg.Row("external_contour_areas[non-zero]", AREAS, tg.B_MASK, lambda m, t, a: list(ct.external_contour_areas(m, t["mask"], -1, K)),
           lambda a: ref_areas(a, -1)),
    tg.Row("enclosing_circle[class 1]", CIRCLE, tg.B_MASK, lambda m, t, a: call_circle(m, t, 1), lambda a: ref_circle(a, 1)),
    tg.Row("measure_diameter[non-zero]", CIRCLE, tg.B_MASK, lambda m, t, a: ct.measure_diameter(m, t["mask"], -1, K),
           lambda a: np.array([2.0 * ct.support_table_np(f, -1)[1][1] for f in a["mask"]])),
    paste_row("paste_roi_masks[inside]", lambda s: (5, 3, s[2], s[1]), lambda s: (s[1] + 7, s[2] + 13)),
    paste_row("paste_roi_masks[overhang]", lambda s: (s[2] - 9, s[1] - 4, s[2], s[1]), lambda s: (s[1] + 1, s[2] + 2)),
    tg.Row("create_overlay_masks", ["unetpp_overlay_chain_u8"], build_overlay,
           lambda m, t, a: ct.create_overlay_masks(m, t["frames"], t["cable"], t["tape"], t["burr"]),
           lambda a: np.stack([ct.create_overlay_masks_np(a["frames"][i], a["cable"][i], a["tape"][i], a["burr"][i]) for i in range(len(a["frames"]))])),
]
ROW_BY_NAME = {r.name: r for r in ROWS_CONTOURS}


@pytest.mark.gpu
@pytest.mark.parametrize("placement", list(tg.PLACEMENTS))
@pytest.mark.parametrize("name", list(ROW_BY_NAME))
def test_row(torch_cuda, model, name, placement):  # noqa: F811
    r = ROW_BY_NAME[name]
    got = tg.run_row(torch_cuda, model, r, placement)
    if placement in tg.SAME_BITS:
        guarded.assert_same_bytes(tg.run_row(torch_cuda, model, r, tg.SAME_BITS[placement]), got,
                                  f"{name}: {tg.SAME_BITS[placement]} (aligned) against {placement} (the pointer says no)")
