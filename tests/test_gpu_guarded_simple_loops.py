"""Guard-band tests of the fifth binding table (include/unetpp_simple_loops.h): every public call of unet_amd/simple_loops.py
between random guard bytes, through the harness and the placements of tests/test_gpu_guarded.py, with its four assertions: guards
intact, equal to the NumPy form bit for bit, the same bits with the filling complemented, placements of one data set bitwise
equal.  The rows live in this module's own list (ROWS_SIMPLE_LOOPS); tests/test_simple_loops_host.py compares it with the table.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded_simple_loops.py -m gpu"""
import numpy as np
import pytest

import guarded
import test_gpu_guarded as tg
from test_gpu_guarded import model, torch_cuda  # noqa: F401  (fixtures)
from unet_amd import simple_loops as sl

K = 1024
CC = ["unetpp_components", "unetpp_components_keep"]
PREDICT = ["unetpp_threshold_classes_f32", "unetpp_merge_classes", "unetpp_mask_join_u8"] + CC


def build_probs(channels, layout="nchw"):
    return lambda s, r: {"probs": sl.make_random_probs(s[0], channels, s[1], s[2], int(r.integers(1 << 30)), True, layout)}


def build_pair(s, r):
    m = tg.class_mask(s, r)
    tape = (m == 2).astype(np.uint8)
    tape[0] *= 3                                              # frame 0: values that are not 0/1 (the areas are sums of values)
    cable = (m == 1).astype(np.uint8) * 255
    cable[-1] = 0                                             # the last frame: no cable
    cable[0, :, : s[2] // 3] = 0
    cable[0, :, 2 * s[2] // 3:] = 0                           # frame 0: a narrow extent, so that the filter removes something
    return {"tape": tape, "cable": cable}


def build_planes(s, r):
    kinds = (sl.PLANE_SCENES * 2)[:s[0]]
    return {"probs": sl.make_simple_batch(kinds, s[1] // 2, s[2] // 2, int(r.integers(1 << 20))), "hw": np.array(s[1:])}


def predict_row(variant, extra):
    kw = dict(sl.SCALED_TAPE)
    return tg.Row(f"predict_simple[{variant}]", PREDICT + extra, build_planes,
                  lambda m, t, a: list(sl.predict_simple(m, t["probs"], a["hw"].tolist(), variant, max_components=K, return_tape_table=variant == "optimized", **kw)),
                  lambda a: list(sl.predict_simple_np(a["probs"], a["hw"].tolist(), variant, return_tape_table=variant == "optimized", **kw)))


ROWS_SIMPLE_LOOPS = [
    tg.Row("relative_threshold[nchw, C=3]", ["unetpp_pixel_rules_f32"], build_probs(3), lambda m, t, a: list(sl.relative_threshold(m, t["probs"])),
           lambda a: list(sl.relative_threshold_np(a["probs"]))),
    tg.Row("relative_threshold[nhwc, C=7]", ["unetpp_pixel_rules_f32"], build_probs(7, "nhwc"),
           lambda m, t, a: list(sl.relative_threshold(m, t["probs"], 1.5, 3.0, "nhwc")), lambda a: list(sl.relative_threshold_np(a["probs"], 1.5, 3.0, "nhwc"))),
    tg.Row("confidence_threshold[nchw, C=7]", ["unetpp_pixel_rules_f32"], build_probs(7), lambda m, t, a: list(sl.confidence_threshold(m, t["probs"], 0.3)),
           lambda a: list(sl.confidence_threshold_np(a["probs"], 0.3))),
    tg.Row("confidence_threshold[nhwc, C=3]", ["unetpp_pixel_rules_f32"], build_probs(3, "nhwc"),
           lambda m, t, a: list(sl.confidence_threshold(m, t["probs"], 0.4, "nhwc")), lambda a: list(sl.confidence_threshold_np(a["probs"], 0.4, "nhwc"))),
    tg.Row("keep_components[class 1]", CC, tg.B_MASK, lambda m, t, a: sl.keep_components(m, t["mask"], 20, 400, 6, match_class=1, out_value=9, max_components=K),
           lambda a: sl.keep_components_np(a["mask"], 20, 400, 6, match_class=1, out_value=9)),
    tg.Row("keep_components[non-zero]", CC, tg.B_MASK, lambda m, t, a: sl.keep_components(m, t["mask"], 2, max_components=K),
           lambda a: sl.keep_components_np(a["mask"], 2)),
    tg.Row("tape_position_filter", ["unetpp_tape_position_filter_u8"], build_pair, lambda m, t, a: list(sl.tape_position_filter(m, t["tape"], t["cable"])),
           lambda a: list(sl.tape_position_filter_np(a["tape"], a["cable"]))),
    tg.Row("column_band", ["unetpp_column_band_u8"], tg.B_MASK, lambda m, t, a: sl.column_band(m, t["mask"]), lambda a: sl.column_band_np(a["mask"])),
    tg.Row("column_band[0.1, 0.95]", ["unetpp_column_band_u8"], tg.B_MASK, lambda m, t, a: sl.column_band(m, t["mask"], 0.1, 0.95),
           lambda a: sl.column_band_np(a["mask"], 0.1, 0.95)),
    tg.Row("threshold_planes", ["unetpp_threshold_classes_f32"], build_planes,
           lambda m, t, a: sl.threshold_planes(m, t["probs"], a["hw"].tolist(), (0.3, 0.55, 0.7)), lambda a: sl.threshold_planes_np(a["probs"], a["hw"].tolist(), (0.3, 0.55, 0.7))),
    predict_row("simple", []),
    predict_row("optimized", ["unetpp_tape_position_filter_u8"]),
    tg.Row("predict_simple_backup", ["unetpp_merge_classes"], lambda s, r: {"mask": tg.class_mask(s, r, 7, 0.05)},
           lambda m, t, a: list(sl.predict_simple_backup(m, t["mask"])), lambda a: list(sl.predict_simple_backup_np(a["mask"]))),
]
ROW_BY_NAME = {r.name: r for r in ROWS_SIMPLE_LOOPS}


@pytest.mark.gpu
@pytest.mark.parametrize("placement", list(tg.PLACEMENTS))
@pytest.mark.parametrize("name", list(ROW_BY_NAME))
def test_row(torch_cuda, model, name, placement):  # noqa: F811
    r = ROW_BY_NAME[name]
    got = tg.run_row(torch_cuda, model, r, placement)
    if placement in tg.SAME_BITS:
        guarded.assert_same_bytes(tg.run_row(torch_cuda, model, r, tg.SAME_BITS[placement]), got,
                                  f"{name}: {tg.SAME_BITS[placement]} (aligned) against {placement} (the pointer says no)")
