"""Guard-band tests: no kernel writes or reads outside its tensors (tests/guarded.py is the harness).

Every public call that reaches a launching symbol of include/unetpp.h runs with each input, output and workspace in an
arena of its own, [guard | payload | guard], all of it random bytes, at three placements:

  P1  2 x 32 x 128, everything 16-byte aligned: one 128 x 32 tile, every width and h * w a multiple of 16 (vector paths)
  P2  the same data; uint8 inputs and outputs one byte off, float32 / int32 inputs 4 bytes off 16: the shape says vector,
      the pointer says no
  P3  3 x 33 x 129, inputs one element off: one tile plus one pixel in both axes, an odd frame stride
  P4  the data of P1 with every input somewhere else modulo 16 (uint8 at 3, 0, 15, ...; float32 at 8, 12, 4, ...) and uint8
      outputs at 15: pointers that disagree with each other, for the kernels that vectorise when theirs agree
  P5  2 x 18 x 20 aligned, P6 the same one element off: the width is a multiple of 4 and not of 16, h * w of 4 and 8 and not
      of 16, for the launches that choose by h * w % 4 and the pointers, below one tile in both axes

and asserts (1) every guard byte intact, (2) the results equal to the reference the family's own GPU test uses, bit for
bit, (3) the same bits with the guards' filling complemented, (4) P1, P2 and P4 (and P5, P6) bitwise equal, and that the symbols the row
declares were the ones called.  The network runs at 1 x 16 x 16, 3 x 16 x 80 and 2 x 48 x 80 with 7 classes instead.
ROWS / NETWORK_SYMBOLS / EXCLUDED are also read by tests/test_guarded_host.py, which compares them with the binding table.
Run on the GPU box:  python -m pytest tests/test_gpu_guarded.py -m gpu"""
import os
import sys

import numpy as np
import pytest

import guarded
from unet_amd import components as cc
from unet_amd import edges as ed
from unet_amd import enhance as en
from unet_amd import evaluation as ev
from unet_amd import geometry as ge
from unet_amd import morphology as mo
from unet_amd import multiclass as mc
from unet_amd import nlmeans as nlm
from unet_amd import probmap as pm
from unet_amd import robust as rb
from unet_amd import tiling as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 1024                                           # max_components of every component row
PLACEMENTS = {"P1": ((2, 32, 128), "aligned"), "P2": ((2, 32, 128), "off"), "P3": ((3, 33, 129), "off"), "P4": ((2, 32, 128), "mixed"),
              "P5": ((2, 18, 20), "aligned"), "P6": ((2, 18, 20), "off")}
SAME_BITS = {"P2": "P1", "P4": "P1", "P6": "P5"}                      # placements of one data set: bitwise equal results
MIXED = {1: (3, 0, 15), 2: (2, 6, 14), 4: (8, 12, 4), 8: (8, 0, 8)}      # P4: the k-th input's address modulo 16, by element size
COLORS = {1: (255, 0, 0), 2: (0, 255, 0), 3: (0, 0, 255), 5: (10, 200, 250), 6: (77, 3, 129)}

# Symbols that write no caller-provided device buffer: load, status, profile, debug, layout and size queries.
EXCLUDED = {
    "unetpp_create": "engine construction", "unetpp_destroy": "engine destruction", "unetpp_last_error": "status text",
    "unetpp_version": "status text", "unetpp_weights_blob_bytes": "size query", "unetpp_weights_blob_bytes_arch": "size query",
    "unetpp_load_weights": "load: writes the engine's own weights", "unetpp_load_weights_device": "load: reads a device blob, writes the engine's own weights",
    "unetpp_workspace_bytes": "size query", "unetpp_status": "status", "unetpp_profile_enable": "profile", "unetpp_profile_count": "profile",
    "unetpp_profile_read": "profile: host buffer", "unetpp_profile_name": "profile", "unetpp_profile_work": "profile",
    "unetpp_profile_plan": "profile: host buffer",
    "unetpp_debug_read": "debug: host buffer", "unetpp_debug_keep_intermediates": "debug", "unetpp_ds_blob_bytes": "size query",
    "unetpp_load_ds_heads": "load: writes the engine's own heads", "unetpp_components_workspace_bytes": "size query",
    "unetpp_morphology_layout": "layout query", "unetpp_canny_workspace_bytes": "size query", "unetpp_canny_layout": "layout query",
    "unetpp_edges_union_workspace_bytes": "size query", "unetpp_enhance_workspace_bytes": "size query", "unetpp_enhance_layout": "layout query",
    "unetpp_nlmeans_layout": "layout query", "unetpp_evaluation_layout": "layout query", "unetpp_probmap_layout": "layout query",
    "unetpp_distance_workspace_bytes": "size query", "unetpp_roi_limit_workspace_bytes": "size query",
    "unetpp_quality_gate_workspace_bytes": "size query", "unetpp_merge_classes_layout": "layout query",
}
NETWORK_SYMBOLS = {"unetpp_forward_ex", "unetpp_forward_ds", "unetpp_forward"}


def orc():
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import unetpp_oracle
    return unetpp_oracle


# ---- data ------------------------------------------------------------------------------------------------------------------------
def class_mask(shape, r, classes=3, speck=0.02):
    """uint8 [B,H,W]: 8 x 8 blocks of random classes, so that components cross rows and tiles, plus single-pixel speckle."""
    B, H, W = shape
    coarse = r.integers(0, classes, (B, (H + 7) // 8, (W + 7) // 8), dtype=np.uint8)
    m = np.repeat(np.repeat(coarse, 8, 1), 8, 2)[:, :H, :W].copy()
    s = r.random(shape) < speck
    m[s] = r.integers(0, classes, int(s.sum()), dtype=np.uint8)
    return m


def gray_frames(shape, r):
    B, H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    g = np.stack([96 + 60 * np.sin(x / (5.0 + b)) * np.cos(y / 4.0) + 40 * ((x // 16 + y // 8 + b) % 2) for b in range(B)])
    return np.clip(g + r.normal(0, 6, shape), 0, 255).astype(np.uint8)


def bgr_frames(shape, r):
    """uint8 [B,H,W,3]: frame 0 grey (three equal channels plus a little noise), the others coloured."""
    g = gray_frames(shape, r)
    f = np.repeat(g[..., None], 3, 3).astype(np.int16)
    f[1:] += r.integers(-60, 60, f[1:].shape, dtype=np.int16)
    f[0] += r.integers(-2, 3, f[0].shape, dtype=np.int16)
    return np.clip(f, 0, 255).astype(np.uint8)


def prob_planes(shape, r):
    """float32 in [0, 1]: smooth blobs plus noise, a few exact 0 and 1."""
    B, H, W = shape[0], shape[-2], shape[-1]
    y, x = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.45 * np.sin(x / 7.0) * np.cos(y / 5.0)
    p = np.clip(base + r.normal(0, 0.08, shape), 0, 1).astype(np.float32)
    flat = p.reshape(-1)
    flat[r.integers(0, flat.size, 8)] = 0.0
    flat[r.integers(0, flat.size, 8)] = 1.0
    return p


def expected_components(masks, connectivity, match_class, k=K):
    B, H, W = masks.shape
    labels, num = np.zeros((B, H, W), np.int32), np.zeros(B, np.int32)
    stats, sums = np.zeros((B, k, 5), np.int32), np.zeros((B, k, 2), np.uint64)
    for b in range(B):
        l, s, sm = cc.components_np(masks[b], connectivity, match_class)
        assert len(s) <= k, "the scene has more components than the rows of this module's tables"
        labels[b], num[b] = l, len(s)
        stats[b, :len(s)], sums[b, :len(s)] = s, sm
    return labels, num, stats, sums


def per_frame(fn, *arrays):
    return np.stack([fn(*a) for a in zip(*arrays)])


# ---- rows ------------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, name, symbols, build, call, ref, align16=(), align=None, exempt=(), shapes=None):
        """build(shape, rng) -> {name: array}; call(model, tensors, arrays) -> results; ref(arrays) -> the same structure in
        NumPy.  align16: inputs the header wants 16-byte aligned; align: guarded.Guard's override for outputs with a
        stricter contract than their element size; exempt: {(entry, argument)} the completeness hook lets through, each
        with its reason beside the row; shapes: {placement: shape} where the row needs its own."""
        self.name, self.symbols, self.build, self.call, self.ref = name, set(symbols), build, call, ref
        self.align16, self.align, self.exempt, self.shapes = set(align16), align, set(exempt), shapes or {}


ROWS = []


def row(*a, **kw):
    ROWS.append(Row(*a, **kw))


B_MASK = lambda s, r: {"mask": class_mask(s, r)}
B_GRAY = lambda s, r: {"gray": gray_frames(s, r)}
B_BGR = lambda s, r: {"frames": bgr_frames(s, r)}
B_GRAY_CABLE = lambda s, r: {"gray": gray_frames(s, r), "cable": (class_mask(s, r, 2, 0.0) != 0).astype(np.uint8)}

# -- mask statistics and the two resizes
row("mask_stats", ["unetpp_mask_stats"], B_MASK, lambda m, t, a: m.mask_stats(t["mask"]), lambda a: orc().mask_stats_np(a["mask"], 3))
row("resize_frames", ["unetpp_resize_linear_u8"], B_BGR, lambda m, t, a: m.resize_frames(t["frames"], (45, 100)),
    lambda a: per_frame(lambda f: orc().cv2_resize_linear_u8_np(f, (100, 45)), a["frames"]))
row("resize_masks", ["unetpp_resize_nearest_roi_u8"], B_MASK, lambda m, t, a: m.resize_masks(t["mask"], (150, 47), 1, (5, 3, 140, 40)),
    lambda a: per_frame(lambda f: orc().clip_to_roi_np(orc().cv2_resize_nearest_np((f == 1).astype(np.uint8), (150, 47)), (5, 3, 140, 40)), a["mask"]))


# -- connected components
def ref_components(a):
    labels, num, stats, sums = expected_components(a["mask"], 8, 1)
    return labels, num, stats, cc.centroids_np(stats, sums)


row("components", ["unetpp_components"], B_MASK, lambda m, t, a: m.components(t["mask"], 1, 8, K), ref_components)
row("components[4-connected, != 0]", ["unetpp_components"], B_MASK, lambda m, t, a: m.components(t["mask"], -1, 4, K)[:3],
    lambda a: expected_components(a["mask"], 4, -1)[:3])
for _rule, _kw in (("largest", dict(min_area=10)), ("spatial", dict(min_area=20, min_width=2, max_width=100, min_height_ratio=0.1)),
                   ("cable_shape", dict(min_area=20, min_aspect=0.5, max_center_offset=0.9))):
    row(f"filter_components[{_rule}]", ["unetpp_components", "unetpp_components_filter"], B_MASK,
        lambda m, t, a, rule=_rule, kw=_kw: m.filter_components(t["mask"], 1, rule, max_components=K, out_value=7, **kw),
        lambda a, rule=_rule, kw=_kw: per_frame(lambda f: cc.filter_components_np(f, 1, rule, 8, 7, **kw), a["mask"]))
row("filter_components_box", ["unetpp_components", "unetpp_components_filter_box"], B_MASK,
    lambda m, t, a: m.filter_components_box(t["mask"], 2, 3, 400, 4.0, 1, max_components=K, out_value=9),
    lambda a: per_frame(lambda f: ed.filter_box_np(f, 2, 3, 400, 4.0, 1, 9), a["mask"]))


# -- morphology
def ref_single(a):
    el, steps, res = mo.program_single("close", mo.structuring_element("ellipse", 5), None, 1)
    return mo.run_program_np(a["mask"], None, el, steps, 1, -1, res, 1)


def _ring():
    return mo.program_ring(5, 3)


row("morphology", ["unetpp_morphology"], B_MASK, lambda m, t, a: m.morphology(t["mask"], 1, "close", 5), ref_single)
row("morphology_program", ["unetpp_morphology"], lambda s, r: {"mask": class_mask(s, r), "other": class_mask(s, r)},
    lambda m, t, a: m.morphology_program(t["mask"], 2, _ring()[1], _ring()[0], t["other"], 1, _ring()[2], 9),
    lambda a: mo.run_program_np(a["mask"], a["other"], _ring()[0], _ring()[1], 2, 1, _ring()[2], 9))
row("morphology[erode, rect 3, twice]", ["unetpp_morphology"], B_MASK, lambda m, t, a: m.morphology(t["mask"], -1, "erode", 3, "rect", 2, out_value=255),
    lambda a: mo.run_program_np(a["mask"], None, *mo.program_single("erode", mo.structuring_element("rect", 3), None, 2)[:2], -1, -1,
                                mo.program_single("erode", mo.structuring_element("rect", 3), None, 2)[2], 255))
row("boundary_band", ["unetpp_morphology"], B_MASK, lambda m, t, a: m.boundary_band(t["mask"], 1, 4, 255),
    lambda a: mo.run_program_np(a["mask"], None, *mo.program_band(4)[:2], 1, -1, mo.program_band(4)[2], 255))
row("constrain_tape_to_ring", ["unetpp_morphology", "unetpp_components", "unetpp_components_filter"], B_MASK,
    lambda m, t, a: m.constrain_tape_to_ring(t["mask"], t["mask"], 2, 1, 7, 3, max_components=K),
    lambda a: per_frame(lambda f: mo.constrain_tape_to_ring_np(f, f, 2, 1, 7, 3), a["mask"]))


def ref_postprocess(a):
    out = [mo.postprocess_masks_np(f, 1, 2, None, min_area=20, min_aspect=0.5, max_center_offset=0.9) for f in a["mask"]]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


row("postprocess_masks", ["unetpp_morphology", "unetpp_components", "unetpp_components_filter"], B_MASK,
    lambda m, t, a: m.postprocess_masks(t["mask"], 1, 2, min_area=20, min_aspect=0.5, max_center_offset=0.9, max_components=K), ref_postprocess)
row("tape_holes", ["unetpp_morphology", "unetpp_components"], B_MASK, lambda m, t, a: m.tape_holes(t["mask"], 2, 3, K),
    lambda a: (np.int64([mo.tape_holes_np(f, 2, 3)[0] for f in a["mask"]]), np.int64([mo.tape_holes_np(f, 2, 3)[1] for f in a["mask"]])))

# -- stage-2 burr detection
T5 = ed.gaussian_taps(5, 1.0)
row("bgr_to_gray", ["unetpp_gray_u8"], B_BGR, lambda m, t, a: m.bgr_to_gray(t["frames"]), lambda a: ed.bgr_to_gray_np(a["frames"]))
row("gaussian_blur", ["unetpp_gaussian_blur_u8"], B_GRAY, lambda m, t, a: m.gaussian_blur(t["gray"], 5, 1.0),
    lambda a: per_frame(lambda f: ed.gaussian_blur_np(f, T5), a["gray"]))
row("canny", ["unetpp_canny_u8"], B_GRAY, lambda m, t, a: m.canny(t["gray"], 50, 150, blur=(5, 1.0)),
    lambda a: per_frame(lambda f: ed.canny_np(ed.gaussian_blur_np(f, T5), 50, 150), a["gray"]))
row("canny[no blur]", ["unetpp_canny_u8"], B_GRAY, lambda m, t, a: m.canny(t["gray"], 40, 120), lambda a: per_frame(lambda f: ed.canny_np(f, 40, 120), a["gray"]))
row("burr_mask_rulebased", ["unetpp_morphology", "unetpp_laplacian_band_u8", "unetpp_components", "unetpp_components_filter_box"], B_GRAY_CABLE,
    lambda m, t, a: m.burr_mask_rulebased(t["gray"], t["cable"], band_out=4, laplacian_threshold=20, min_area=2, max_area=500, max_components=K),
    lambda a: per_frame(lambda g, c: ed.burr_mask_rulebased_np(g, c, band_out=4, laplacian_threshold=20, min_area=2, max_area=500), a["gray"], a["cable"]))
_DB = dict(min_area=2, max_area=800, band_ksize=8, max_aspect=50.0, min_side=0, canny_low=30, canny_high=90)
row("detect_burrs", ["unetpp_canny_u8", "unetpp_morphology", "unetpp_components", "unetpp_components_filter_box"], B_GRAY_CABLE,
    lambda m, t, a: m.detect_burrs(t["gray"], t["cable"], max_components=K, **_DB),
    lambda a: per_frame(lambda g, c: ed.detect_burrs_np(g, c, **_DB), a["gray"], a["cable"]))
row("edges_combined", ["unetpp_canny_u8", "unetpp_edges_union_u8"], B_GRAY, lambda m, t, a: m.edges_combined(t["gray"]),
    lambda a: per_frame(lambda f: ed.edges_combined_np(f, ed.canny_np(ed.gaussian_blur_np(f, T5), 30, 100)), a["gray"]))
row("dog_band", ["unetpp_dog_band_u8"], B_GRAY_CABLE, lambda m, t, a: m.dog_band(t["gray"], t["cable"], threshold=5),
    lambda a: per_frame(lambda g, b: np.where((b != 0) & (ed.dog_u8_np(g) > ed._u8_threshold(5)), np.uint8(255), np.uint8(0)), a["gray"], a["cable"]))
row("count_nonzero", ["unetpp_count_nonzero_u8"], B_MASK, lambda m, t, a: m.count_nonzero(t["mask"]),
    lambda a: np.int32([np.count_nonzero(f) for f in a["mask"]]))

# -- measurements
row("row_widths", ["unetpp_row_widths"], B_MASK, lambda m, t, a: m.row_widths(t["mask"], 1, t["mask"], 2), lambda a: ge.row_widths_np(a["mask"], 1, a["mask"], 2))


def build_widths(s, r):
    w = r.integers(0, 40, (s[0], 2, s[2])).astype(np.float32)          # rows = this placement's width: 128 / 129
    w[:, :, ::7] = 0
    return {"widths": w}


def ref_profile(a):
    taps = ge.gaussian_taps_f32(5)
    out = [ge.width_profile_np(x, taps, 3) for x in a["widths"]]
    return (np.stack([o[0] for o in out]), np.stack([o[1].astype(np.uint8) for o in out]), np.stack([o[0][1] - o[0][0] for o in out]),
            np.float32([o[2] for o in out]), np.float32([o[3] for o in out]), np.int32([o[4] for o in out]))


row("width_profile", ["unetpp_width_profile"], build_widths, lambda m, t, a: m.width_profile(t["widths"], 5, 3), ref_profile)


def build_summary(s, r):
    _, num, stats, _ = expected_components(class_mask(s, r), 8, 1)
    return {"num": num, "stats": stats}


row("components_summary", ["unetpp_components_summary"], build_summary, lambda m, t, a: m.components_summary(t["num"], t["stats"], 3),
    lambda a: per_frame(lambda n, st: ge.components_summary_np(n, st, 3), a["num"], a["stats"]))


# -- sliding-window inference: patch_size 32, stride 16, target_size 16
def n_patches(s):
    return tl.tile_plan(s[1], s[2], 32, 16).n_patches


def build_maps(s, r):
    n = s[0] * n_patches(s)
    inc = (r.random(n) < 0.7).astype(np.uint8)
    inc[0] = 0
    return {"maps": r.standard_normal((n, 3, 16, 16)).astype(np.float32), "include": inc, "hw": np.int64(s[1:])}


def ref_gather(a):
    f = a["frames"]
    plan = tl.tile_plan(f.shape[1], f.shape[2], 32, 16)
    return np.concatenate([tl.gather_tiles_np(x, plan, 32, 16, "rgb") for x in f])


def ref_gate(a):
    inc, scores = tl.tile_gate_np(a["maps"], 0.5, 1)
    return inc.astype(np.uint8), scores


def ref_blend(a):
    h, w = (int(v) for v in a["hw"])
    plan = tl.tile_plan(h, w, 32, 16)
    p = plan.n_patches
    out = [tl.blend_tiles_np(a["maps"][i:i + p], plan, h, w, 32, include=a["include"][i:i + p] != 0) for i in range(0, len(a["maps"]), p)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


row("gather_tiles", ["unetpp_tile_gather_u8"], B_BGR, lambda m, t, a: m.gather_tiles(t["frames"], 32, 16, 16, "rgb"), ref_gather)
row("gather_tiles[bgr]", ["unetpp_tile_gather_u8"], B_BGR, lambda m, t, a: m.gather_tiles(t["frames"], 32, 16, 16, "bgr"),
    lambda a: np.concatenate([tl.gather_tiles_np(x, tl.tile_plan(x.shape[0], x.shape[1], 32, 16), 32, 16, "bgr") for x in a["frames"]]))
row("blend_tiles[no gate, mask only]", ["unetpp_tile_blend_f32"], build_maps,
    lambda m, t, a: m.blend_tiles(t["maps"], tuple(int(v) for v in a["hw"]), 32, 16, None, False)[0],
    lambda a: ref_blend(dict(a, include=np.ones_like(a["include"])))[0])
row("tile_gate", ["unetpp_tile_gate_f32"], build_maps, lambda m, t, a: m.tile_gate(t["maps"], 0.5, 1), ref_gate,
    align16=["maps"])                                                # include/unetpp.h: dev_maps 16-byte aligned
row("blend_tiles", ["unetpp_tile_blend_f32"], build_maps,
    lambda m, t, a: m.blend_tiles(t["maps"], tuple(int(v) for v in a["hw"]), 32, 16, t["include"]), ref_blend)

# -- grey-frame enhancement: CLAHE with tile_grid (2, 2)
LUTS4 = lambda shape, dtype, ctx: 4 if len(shape) == 3 and shape[-1] == 256 else None      # dev_luts: uint8, 4-byte aligned
row("is_grayscale", ["unetpp_gray_decision"], B_BGR, lambda m, t, a: m.is_grayscale(t["frames"], 10.0, True),
    lambda a: (np.array([en.is_grayscale_np(f) for f in a["frames"]]), np.int64([en.channel_diff_sums(f) for f in a["frames"]])))


def ref_clahe(a):
    out = [en.clahe_np(g, 2.0, (2, 2), return_luts=True) for g in a["gray"]]
    return np.stack([o[0] for o in out]), np.stack([np.asarray(o[1], np.uint8).reshape(4, 256) for o in out])


def call_clahe_entry(m, t, a):
    """unetpp_clahe_u8 has no wrapper of its own (clahe() runs the fused entry): through _call, as the wrappers call."""
    import torch
    from unet_amd import _lib
    g = m._input(t["gray"])
    b, h, w = g.shape
    ws = m._workspace(("enhance", b, h, w, 2, 2), lambda: _lib.load().unetpp_enhance_workspace_bytes(b, h, w, 2, 2), g.device, "clahe: unsupported")
    out = torch.empty_like(g)
    luts = torch.empty((b, 4, 256), dtype=torch.uint8, device=g.device)
    m._call("unetpp_clahe_u8", g, b, h, w, 2.0, 2, 2, out, luts, ws, stream_of=g)
    return out, luts


row("clahe", ["unetpp_enhance_u8"], B_GRAY, lambda m, t, a: m.clahe(t["gray"], 2.0, (2, 2), return_luts=True), ref_clahe, align=LUTS4)
row("clahe_entry", ["unetpp_clahe_u8"], B_GRAY, call_clahe_entry, ref_clahe, align=LUTS4)
row("bilateral_filter", ["unetpp_bilateral_u8"], B_GRAY, lambda m, t, a: m.bilateral_filter(t["gray"]), lambda a: per_frame(en.bilateral_np, a["gray"]))
row("enhance_grayscale", ["unetpp_enhance_u8"], B_BGR, lambda m, t, a: m.enhance_grayscale(t["frames"], tile_grid=2),
    lambda a: per_frame(lambda f: en.enhance_grayscale_np(f, tile_grid=2), a["frames"]))
row("enhance_grayscale[grey in, one channel out]", ["unetpp_enhance_u8"], B_GRAY, lambda m, t, a: m.enhance_grayscale(t["gray"], tile_grid=2, channels_out=1),
    lambda a: per_frame(lambda f: en.enhance_grayscale_np(f, tile_grid=2, channels_out=1), a["gray"]))
row("preprocess_frames", ["unetpp_enhance_u8"], B_BGR, lambda m, t, a: m.preprocess_frames(t["frames"], tile_grid=2, return_decisions=True),
    lambda a: (per_frame(lambda f: en.preprocess_frame_np(f, True, 10.0, tile_grid=2), a["frames"]), np.array([en.is_grayscale_np(f) for f in a["frames"]])))

# -- non-local means: its tile is 64 wide and 128 high; the weight table is a cached read-only device tensor built with
#    torch.from_numpy(...).to(device), which the allocation patch does not see: argument 7 is exempt
row("nl_means", ["unetpp_nlmeans_u8"], B_GRAY, lambda m, t, a: nlm.nl_means(m, t["gray"]), lambda a: per_frame(nlm.nl_means_np, a["gray"]),
    exempt=[("unetpp_nlmeans_u8", 7)], shapes={"P3b": (2, 129, 65)})

# -- evaluation
B_EVAL = lambda s, r: {"pred": class_mask(s, r), "target": np.where(r.random(s) < 0.03, np.uint8(255), class_mask(s, r))}
row("confusion", ["unetpp_confusion_u8"], B_EVAL, lambda m, t, a: ev.confusion(m, t["pred"], t["target"], 3, 255), lambda a: ev.confusion_np(a["pred"], a["target"], 3, 255))


def ref_confusion_total(a):
    total = a["total"].copy()
    return ev.confusion_np(a["pred"], a["target"], 3, 255, total=total) + (total,)


row("confusion[total]", ["unetpp_confusion_u8"], lambda s, r: dict(B_EVAL(s, r), total=r.integers(0, 1 << 40, 11, dtype=np.int64)),
    lambda m, t, a: ev.confusion(m, t["pred"], t["target"], 3, 255, total=t["total"]) + (t["total"],), ref_confusion_total)


def build_disagree(s, r):
    a = class_mask(s, r)
    b = np.where(r.random(s) < 0.1, class_mask(s, r), a)
    lg = r.standard_normal((s[0], 3, s[1], s[2])).astype(np.float32)
    lg[0, 1, 3, 5] = np.nan
    b[0, 3, 5] = (a[0, 3, 5] + 1) % 3
    return {"a": a, "b": b, "logits": lg}


row("confusion[no ignore]", ["unetpp_confusion_u8"], lambda s, r: {"pred": class_mask(s, r, 4), "target": class_mask(s, r, 4)},
    lambda m, t, a: ev.confusion(m, t["pred"], t["target"], 3, check=False), lambda a: ev.confusion_np(a["pred"], a["target"], 3))
row("mask_disagreement[no logits]", ["unetpp_mask_disagreement"], build_disagree, lambda m, t, a: ev.mask_disagreement(m, t["a"], t["b"]),
    lambda a: ev.disagreement_np(a["a"], a["b"]))
row("mask_disagreement", ["unetpp_mask_disagreement"], build_disagree, lambda m, t, a: ev.mask_disagreement(m, t["a"], t["b"], t["logits"]),
    lambda a: ev.disagreement_np(a["a"], a["b"], a["logits"]))

# -- the robust loop's mask rules
B_PAIR = lambda s, r: {"mask": (r.random(s) >= 0.05).astype(np.uint8) * r.integers(1, 3, s, dtype=np.uint8), "other": (r.random(s) < 0.6).astype(np.uint8) * 3}
row("distance_transform", ["unetpp_distance_transform_u8"], B_PAIR, lambda m, t, a: rb.distance_transform(m, t["mask"]),
    lambda a: per_frame(rb.distance_transform_np, a["mask"] != 0))
for _metric, _inv in (("l1", True), ("c", False)):
    row(f"distance_transform[{_metric}]", ["unetpp_distance_transform_u8"], B_PAIR,
        lambda m, t, a, metric=_metric, inv=_inv: rb.distance_transform(m, t["mask"], 2, inv, metric),
        lambda a, metric=_metric, inv=_inv: per_frame(lambda f: rb.distance_transform_np(f, metric), (a["mask"] == 2) != inv))
row("distance_ring", ["unetpp_distance_transform_u8"], B_PAIR,
    lambda m, t, a: rb.distance_ring(m, t["mask"], t["other"], 1, 4, invert=False, match1=3, return_distance=True),
    lambda a: (per_frame(lambda f, o: rb.ring_np(f, o == 3, 1, 4), a["mask"] != 0, a["other"]), per_frame(rb.distance_transform_np, a["mask"] != 0)))
row("keep_best_cable", ["unetpp_components", "unetpp_components_best_cable"], lambda s, r: {"mask": class_mask(s, r, 2, 0.01)},
    lambda m, t, a: rb.keep_best_cable(m, t["mask"], 10, 0.1, 0.5, 0.9, max_components=K),
    lambda a: per_frame(lambda f: rb.keep_best_cable_np(f, 10, 0.1, 0.5, 0.9), a["mask"]))


def build_roi(s, r):
    cable = np.zeros(s, np.uint8)
    cable[:, 5:20, 30:41] = 1
    cable[-1] = 0                                                   # an empty cable empties its frame
    return {"mask": (r.random(s) < 0.5).astype(np.uint8), "cable": cable}


row("roi_limit", ["unetpp_roi_limit_u8"], build_roi, lambda m, t, a: rb.roi_limit(m, t["mask"], t["cable"], 2),
    lambda a: per_frame(lambda g, c: rb.roi_limit_np(g, c, 2), a["mask"], a["cable"]))
row("row_width_median", ["unetpp_row_widths", "unetpp_row_width_median"], lambda s, r: {"cable": class_mask(s, r, 2), "tape": class_mask(s, r, 2)},
    lambda m, t, a: rb.measure_robust(m, t["cable"], t["tape"]), lambda a: [rb.measure_diameters_np(c, t) for c, t in zip(a["cable"], a["tape"])])
row("letterbox", ["unetpp_resize_linear_u8"], B_BGR, lambda m, t, a: rb.letterbox(m, t["frames"], 64)[0],
    lambda a: per_frame(lambda f: rb.letterbox_np(f, 64)[0], a["frames"]))
# unletterbox_masks hands resize_masks `masks[:, top:.., left:..].contiguous()`, a copy torch makes itself: argument 0 exempt
row("unletterbox_masks", ["unetpp_resize_nearest_roi_u8"], lambda s, r: {"masks": class_mask((s[0], 64, 64), r), "hw": np.int64(s[1:])},
    lambda m, t, a: rb.unletterbox_masks(m, t["masks"], rb.letterbox_plan(int(a["hw"][0]), int(a["hw"][1]), 64)),
    lambda a: per_frame(lambda f: rb.unletterbox_mask_np(f, rb.letterbox_plan(int(a["hw"][0]), int(a["hw"][1]), 64)), a["masks"]),
    exempt=[("unetpp_resize_nearest_roi_u8", 0)])

# -- probability-map rules: the plane is channel 1 of an [B,H,W,2] tensor (pixel stride 2) or a plain [B,H,W]
THR = [0.2, 0.5, 0.7, 0.9]
B_PROB = lambda s, r: {"prob": prob_planes(s, r)}
row("threshold_levels", ["unetpp_prob_levels_f32"], lambda s, r: {"prob": np.ascontiguousarray(np.stack([prob_planes(s, r), prob_planes(s, r)], -1))},
    lambda m, t, a: pm.threshold_levels(m, t["prob"], 0.3, 0.7, channel=1), lambda a: pm.levels_np(a["prob"], 0.3, 0.7, channel=1))
row("threshold_levels[plane]", ["unetpp_prob_levels_f32"], B_PROB, lambda m, t, a: pm.threshold_levels(m, t["prob"], 0.3, 0.7),
    lambda a: pm.levels_np(a["prob"], 0.3, 0.7))


def build_hist(s, r):
    return {"prob": prob_planes(s, r), "target": np.where(r.random(s) < 0.03, np.uint8(255), class_mask(s, r, 2)),
            "total": r.integers(0, 1 << 40, 2 * (len(THR) + 1) + 1, dtype=np.int64)}


def ref_hist(a):
    total = a["total"].copy()
    return pm.threshold_hist_np(a["prob"], a["target"], THR, -1, 255, total, return_outside=True) + (total,)


row("threshold_histogram", ["unetpp_prob_threshold_hist_f32"], build_hist,
    lambda m, t, a: pm.threshold_histogram(m, t["prob"], t["target"], THR, -1, 255, t["total"], return_outside=True) + (t["total"],), ref_hist)


def build_sums(s, r):
    labels, num, _, _ = expected_components(class_mask(s, r), 8, 1)
    return {"labels": labels, "num": num, "prob": prob_planes(s, r)}


row("component_prob_sums", ["unetpp_components_prob_sum_f32"], build_sums, lambda m, t, a: pm.component_prob_sums(m, t["labels"], t["num"], t["prob"], None, K),
    lambda a: pm.prob_sums_np(a["labels"], a["prob"], K))
row("filter_by_mean_prob", ["unetpp_morphology", "unetpp_components", "unetpp_components_prob_sum_f32", "unetpp_components_filter_mean"],
    lambda s, r: {"mask": (class_mask(s, r) != 0).astype(np.uint8), "prob": prob_planes(s, r)},
    lambda m, t, a: pm.filter_by_mean_prob(m, t["mask"], t["prob"], 5, 0.4, 3, max_components=K), lambda a: pm.filter_mean_prob_np(a["mask"], a["prob"], 5, 0.4, 3))

# -- the 6- and 7-class video loops
row("quality_gate", ["unetpp_quality_gate_u8"], lambda s, r: {"frames": bgr_frames(s, r), "prev": gray_frames(s, r)[0]},
    lambda m, t, a: mc.quality_gate(m, t["frames"], t["prev"]), lambda a: mc.quality_gate_np(a["frames"], a["prev"]))
row("quality_gate[first batch]", ["unetpp_quality_gate_u8"], B_BGR, lambda m, t, a: mc.quality_gate(m, t["frames"]), lambda a: mc.quality_gate_np(a["frames"]))
row("merge_classes[bit map]", ["unetpp_merge_classes"], lambda s, r: {"mask": class_mask(s, r, 32, 0.05)},
    lambda m, t, a: mc.merge_classes(m, t["mask"], mc.PLANES_V3, lut=mc.LUT_BITS, num_classes=7),
    lambda a: mc.merge_classes_np(a["mask"], mc.PLANES_V3, lut=mc.LUT_BITS, num_classes=7))
row("merge_classes", ["unetpp_merge_classes"], lambda s, r: {"mask": class_mask(s, r, 7)},
    lambda m, t, a: mc.merge_classes(m, t["mask"], mc.PLANES_VIDEO, num_classes=7), lambda a: mc.merge_classes_np(a["mask"], mc.PLANES_VIDEO, num_classes=7))
B_PROBS6 = lambda s, r: {"probs": prob_planes((s[0], 6, s[1], s[2]), r)}
row("threshold_classes", ["unetpp_threshold_classes_f32"], B_PROBS6, lambda m, t, a: mc.threshold_classes(m, t["probs"]), lambda a: mc.threshold_classes_np(a["probs"]))
row("threshold_classes[resized]", ["unetpp_threshold_classes_f32"], B_PROBS6, lambda m, t, a: mc.threshold_classes(m, t["probs"], (47, 150)),
    lambda a: mc.threshold_classes_np(a["probs"], (47, 150)))
for _mode in ("region", "weighted"):
    row(f"overlay[{_mode}]", ["unetpp_overlay_u8"], lambda s, r: {"frames": bgr_frames(s, r), "mask": class_mask(s, r, 7)},
        lambda m, t, a, mode=_mode: mc.overlay(m, t["frames"], t["mask"], COLORS, 0.6, mode, 7),
        lambda a, mode=_mode: mc.overlay_np(a["frames"], a["mask"], COLORS, 0.6, mode, 7))

ROW_BY_NAME = {r.name: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS)


# ---- running a row -----------------------------------------------------------------------------------------------------------------
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
    return NestedUNet(3, max_batch=1, max_hw=(16, 16)).to("cuda:0")      # no weights: post-processing needs none


def to_numpy(torch, r):
    if isinstance(r, torch.Tensor):
        return r.detach().cpu().numpy()
    if isinstance(r, dict):
        return {k: to_numpy(torch, v) for k, v in r.items()}
    if isinstance(r, (tuple, list)):
        return [to_numpy(torch, v) for v in r]
    return r


def assert_equal(got, want, path):
    """Integers as integers, floats bit for bit (NaN where NaN), containers member by member."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), (path, got, want)
        for k in want:
            assert_equal(got[k], want[k], f"{path}[{k!r}]")
    elif isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), (path, type(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            assert_equal(g, w, f"{path}[{i}]")
    elif isinstance(want, np.ndarray) or isinstance(got, np.ndarray):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (path, got.shape, want.shape)
        if got.dtype.kind == "f":
            want = want.astype(got.dtype)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), f"{path}: NaN in other places"
            u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
            bad = (np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)) & ~nan
        else:
            bad = got.astype(np.int64) != want.astype(np.int64)
        assert not bad.any(), f"{path}: {int(bad.sum())} of {bad.size} values differ from the reference, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"
    else:
        assert got == want, (path, got, want)


_ran = {}


def input_offset(mode, i, array, wants16):
    """The address modulo 16 of the i-th input: 0, one element off, or P4's scatter; 0 where the header demands 16 bytes."""
    if mode == "aligned" or wants16:
        return 0
    return array.dtype.itemsize if mode == "off" else MIXED[array.dtype.itemsize][i % 3]


def run_row(torch, model, r, placement):
    """The four assertions of one row at one placement; returns the bytes of its results (cached for P1 against P2)."""
    from unet_amd import _lib
    if (r.name, placement) in _ran:
        return _ran[(r.name, placement)]
    shape, mode = PLACEMENTS[placement] if placement in PLACEMENTS else (r.shapes[placement], "off")
    arrays = r.build(shape, np.random.default_rng(1000 * shape[1] + shape[2] + len(r.name)))
    seen = {}

    def run(g):
        g.exempt |= r.exempt
        t = {k: g.place(v, input_offset(mode, i, v, k in r.align16), name=k) for i, (k, v) in enumerate(arrays.items()) if k != "hw"}
        with g.allocations(models=[model], lib_module=_lib):
            out = r.call(model, t, arrays)
            torch.cuda.synchronize()
        seen["symbols"] = set(g.symbols) - set(EXCLUDED)
        seen["out"] = to_numpy(torch, out)
        for k, v in t.items():                                       # inputs are read-only, bar the running totals
            if k != "total":
                assert v.cpu().numpy().tobytes() == arrays[k].tobytes(), f"{r.name}: input {k!r} was written"
        return out

    got = guarded.two_fillings(torch, run, seed=len(r.name), u8_out_offset={"aligned": 0, "off": 1, "mixed": 15}[mode], align=r.align)
    assert seen["symbols"] == r.symbols, f"{r.name}: called {sorted(seen['symbols'])}, the row declares {sorted(r.symbols)}"
    assert_equal(seen["out"], to_numpy(torch, r.ref(arrays)), r.name)
    _ran[(r.name, placement)] = got
    return got


def test_the_checks_can_fail_on_device_memory(torch_cuda):
    """The negative controls of tests/test_guarded_host.py once more where the kernels run: a torch write one byte past a
    guarded output (inside the arena's own allocation, no kernel of the project) is caught, an honest copy is not."""
    torch = torch_cuda

    def body(g, overrun):
        x = g.place(np.arange(64, dtype=np.uint8).reshape(2, 32), 1)
        with g.allocations():
            out = torch.empty_like(x)
        out.copy_(x)
        if overrun:
            torch.as_strided(out, (out.numel() + 1,), (1,))[-1] = 7
        return out

    guarded.two_fillings(torch, lambda g: body(g, False), u8_out_offset=1)
    with pytest.raises(guarded.GuardError, match=r"back guard changed, payload-relative offsets 64 \.\. 64"):
        guarded.two_fillings(torch, lambda g: body(g, True), u8_out_offset=1)


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("name", list(ROW_BY_NAME))
def test_row(torch_cuda, model, name, placement):
    r = ROW_BY_NAME[name]
    got = run_row(torch_cuda, model, r, placement)
    if placement in SAME_BITS:
        guarded.assert_same_bytes(run_row(torch_cuda, model, r, SAME_BITS[placement]), got,
                                  f"{name}: {SAME_BITS[placement]} (aligned) against {placement} (the pointer says no)")


@pytest.mark.parametrize("name,placement", [(r.name, p) for r in ROWS for p in r.shapes])
def test_row_at_its_own_shape(torch_cuda, model, name, placement):
    run_row(torch_cuda, model, ROW_BY_NAME[name], placement)


# ---- the network: 7 classes, every tile partial in both axes ----------------------------------------------------------------------------
NET_SHAPES = [(1, 16, 16), (3, 16, 80), (2, 48, 80)]
NET_MODELS = [("nested", "exact"), ("nested", "exact8"), ("nested", "fast"), ("simple", "exact")]
TOL = {"exact": 2e-5, "exact8": 1e-3, "fast": 5e-2}               # the bars of test_gpu_parity.py / test_gpu_exact8.py
RULE = dict(t_cable=0.2, t_tape=0.2, bg_margin=0.05, ct_margin=0.02)
_nets, _refs = {}, {}


def net_model(arch, precision):
    from unet_amd import synthetic as syn
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    if (arch, precision) not in _nets:
        if arch == "nested":
            sd = syn.make_state_dict(7, 3, True, 2)
            m = NestedUNet(7, deep_supervision=True, precision=precision, max_batch=3, max_hw=(48, 80)).to("cuda:0")
        else:
            sd = syn.make_simple_state_dict(7, 3, 2)
            m = SimpleUNet(7, precision=precision, max_batch=3, max_hw=(48, 80)).to("cuda:0")
        m.load_state_dict(sd, strict=True)
        _nets[(arch, precision)] = (m.eval(), sd)
    return _nets[(arch, precision)]


def net_reference(arch, sd, shape):
    """The oracle's logits [out, out1, out2, out3] (out alone for SimpleUNet) and the frames, once per shape."""
    import torch
    import torch.nn.functional as F
    from unet_amd import synthetic as syn
    if (arch, shape) not in _refs:
        B, H, W = shape
        frames = syn.make_frames_u8(B, H, W, "smooth", 7)
        x = syn.frames_to_chw_f32(frames)
        if arch == "simple":
            outs = [orc().simple_unet_torch_forward(sd, x)]
        else:
            logits, t = orc().torch_forward(sd, x, return_intermediates=True)
            outs = [logits]
            for head, node in (("ds1_3", "x1_3"), ("ds2_2", "x2_2"), ("ds3_1", "x3_1")):
                low = F.conv2d(torch.from_numpy(t[node]), torch.from_numpy(sd[head + ".weight"]), torch.from_numpy(sd[head + ".bias"]))
                outs.append(F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).numpy())
        _refs[(arch, shape)] = (frames, x, [np.asarray(o, np.float32) for o in outs])
    return _refs[(arch, shape)]


def check_logits(got, ref, tol, what):
    err = float(np.abs(got - ref).max())
    print(f"{what}: max|dlogit| = {err:.3e} (bar {tol:g})")
    # 'exact' is held relative to the largest logit (test_gpu_parity.py, test_gpu_exact8.py), the other two absolutely
    assert err < (tol * max(1.0, float(np.abs(ref).max())) if tol == TOL["exact"] else tol), (what, err)
    return err


def check_mask(mask, ref_logits, err, what):
    ref_mask = orc().masks_from_logits(ref_logits)[0]
    flips = mask != ref_mask
    assert not (flips & (orc().top2_margin(ref_logits) > 2 * err + 1e-7)).any(), f"{what}: a flipped pixel is not a near-tie"


@pytest.mark.parametrize("shape", NET_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("arch,precision", NET_MODELS)
def test_network(torch_cuda, arch, precision, shape):
    """uint8 frames at an odd byte offset, float32 input 4 bytes off 16, outputs at their contractual alignment (logits and
    probabilities 16, masks 4): guards, the suite's bars against the oracle, status() == 0 and the same bits under both fillings."""
    torch = torch_cuda
    from unet_amd import _lib
    model, sd = net_model(arch, precision)
    frames, x, refs = net_reference(arch, sd, shape)
    tol = TOL[precision]
    nested = arch == "nested"
    seen = {}

    def run(g):
        xf, xu = g.place(x, 4, "x"), g.place(frames, 1, "frames")
        model.status(clear=True)
        with g.allocations(models=[model], lib_module=_lib):
            out = {"forward": model.forward(xf), "segment": model.segment(xu, return_logits=True, return_class_masks=True),
                   "proba": model.predict_proba(xf), "thresholded": model.segment_thresholded(xu, "exclusive", return_probs=True, **RULE)}
            if nested:
                out["ds"] = model.forward_deep_supervision(xf)
                out["pruned"] = [model.forward(xf, output=k) for k in (1, 2, 3)]
                out["segment2"] = model.segment(xu, output=2)
                out["proba3"] = model.predict_proba(xf, output=3)
            torch.cuda.synchronize()
        assert model.status() == 0, "random guard bytes reached the activations"
        seen["symbols"] = set(g.symbols) - set(EXCLUDED)
        seen["out"] = to_numpy(torch, out)
        assert np.array_equal(xf.cpu().numpy(), x) and np.array_equal(xu.cpu().numpy(), frames)
        return out

    guarded.two_fillings(torch, run, seed=shape[2])
    assert seen["symbols"] == ({"unetpp_forward_ex", "unetpp_forward_ds"} if nested else {"unetpp_forward_ex"}), seen["symbols"]
    out, tag = seen["out"], f"{arch} {precision} {shape}"
    err = check_logits(out["forward"], refs[0], tol, tag + " forward")
    mask, cable, tape, logits = out["segment"]
    e2 = check_logits(logits, refs[0], tol, tag + " segment(uint8 frames)")
    check_mask(mask, refs[0], max(err, e2), tag + " segment")
    assert np.array_equal(cable, (mask == 1).astype(np.uint8)) and np.array_equal(tape, (mask == 2).astype(np.uint8))
    ref_p = orc().softmax_np(refs[0], 1)
    perr = float(np.abs(out["proba"] - ref_p).max())
    assert perr < tol, (tag, perr)
    c, t, probs = out["thresholded"]
    assert float(np.abs(probs - ref_p).max()) < tol
    rc, rt, _ = orc().rule_masks_from_logits(refs[0], "exclusive", **RULE)
    p0, p1, p2 = ref_p[:, 0], ref_p[:, 1], ref_p[:, 2]
    d = np.minimum.reduce([np.abs(p1 - RULE["t_cable"]), np.abs(p2 - RULE["t_tape"]), np.abs(p1 - p0 - RULE["bg_margin"]),
                           np.abs(p2 - p0 - RULE["bg_margin"]), np.abs(p0 - RULE["bg_margin"]), np.abs(p1 - p2 - RULE["ct_margin"]),
                           np.abs(p2 - p1 - RULE["ct_margin"]), np.abs(p1 - p2), np.abs(p1 - p0), np.abs(p2 - p0)])
    diff = (c != rc) | (t != rt)
    assert not (diff & (d > 2 * max(perr, 1e-6))).any(), f"{tag}: a rule mask differs away from every decision boundary"
    if nested:
        errs = [check_logits(out["ds"][k], refs[k], tol, f"{tag} ds out{k}") for k in range(4)]
        for k in (1, 2, 3):
            assert np.array_equal(out["pruned"][k - 1].view(np.uint32), out["ds"][k].view(np.uint32)), f"{tag}: pruned output {k} differs from the full pass"
        check_mask(out["segment2"], refs[2], errs[2], tag + " segment(output=2)")
        assert float(np.abs(out["proba3"] - orc().softmax_np(refs[3], 1)).max()) < tol


def test_legacy_forward_entry(torch_cuda):
    """unetpp_forward, the entry without an outputs record, has no wrapper: through _call, guarded like the others."""
    torch = torch_cuda
    from unet_amd import _lib
    model, sd = net_model("nested", "exact")
    shape = NET_SHAPES[1]
    frames, x, refs = net_reference("nested", sd, shape)
    B, H, W = shape
    seen = {}

    def run(g):
        xu = g.place(frames, 1, "frames")
        with g.allocations(models=[model], lib_module=_lib):
            with g.context(guarded.NETWORK):
                xin, fmt, b, h, w = model._prepare(xu)
                logits = torch.empty((b, 7, h, w), dtype=torch.float32, device=xu.device)
                mask, cable, tape = (torch.empty((b, h, w), dtype=torch.uint8, device=xu.device) for _ in range(3))
            model._call("unetpp_forward", xin, fmt, b, h, w, logits, mask, cable, tape, stream_of=xin)
            torch.cuda.synchronize()
        seen["symbols"] = set(g.symbols) - set(EXCLUDED)
        seen["out"] = to_numpy(torch, (logits, mask, cable, tape))
        return logits, mask, cable, tape

    guarded.two_fillings(torch, run, seed=5)
    assert seen["symbols"] == {"unetpp_forward"}
    logits, mask, cable, tape = seen["out"]
    err = check_logits(logits, refs[0], TOL["exact"], "unetpp_forward")
    check_mask(mask, refs[0], err, "unetpp_forward")
    assert np.array_equal(cable, (mask == 1).astype(np.uint8)) and np.array_equal(tape, (mask == 2).astype(np.uint8))
