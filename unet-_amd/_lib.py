"""ctypes binding of the C ABI declared in include/unetpp.h, plus the in-tree build of the HIP library.

The product path has no CPU fallback: if libunetpp_hip.so is missing or cannot be loaded, or no HIP
device is present, every entry point raises."""
from __future__ import annotations

import ctypes
import hashlib
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libunetpp_hip.so")
CSRC = os.path.join(_HERE, "csrc")
SOURCES = ["unetpp_abi.hip", "unetpp_postproc.hip"]      # the engine; the post-processing entry points
INCLUDE = os.path.join(_HERE, "..", "include")
# every header on disk is a build input: source_hash() covers each of them, so a new header cannot leave a stale library looking current
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [
    os.path.join("..", "..", "include", f) for f in sorted(os.listdir(INCLUDE)) if f.endswith(".h")]

STATUS_OVERFLOW, STATUS_NAN = 1, 2
PREC_EXACT, PREC_FAST, PREC_EXACT8 = 0, 1, 2
PRECISIONS = {"exact": PREC_EXACT, "fast": PREC_FAST, "exact8": PREC_EXACT8}
ARCH_NESTED, ARCH_SIMPLE = 0, 1
IN_F32_NCHW, IN_U8_NHWC_BGR = 0, 1


class Config(ctypes.Structure):
    _fields_ = [("num_classes", ctypes.c_int), ("in_channels", ctypes.c_int), ("max_batch", ctypes.c_int),
                ("max_h", ctypes.c_int), ("max_w", ctypes.c_int), ("precision", ctypes.c_int),
                ("device", ctypes.c_int), ("micro_batch", ctypes.c_int), ("streams", ctypes.c_int), ("arch", ctypes.c_int)]


class CcRule(ctypes.Structure):
    """unetpp_cc_rule: the parameters of the component filters (all doubles)."""
    _fields_ = [(n, ctypes.c_double) for n in ("min_area", "min_width", "max_width", "min_height_ratio", "min_aspect",
                                               "max_center_offset", "roi_width")]


CC_RULES = {"largest": 0, "spatial": 1, "cable_shape": 2}


class CcBoxRule(ctypes.Structure):
    """unetpp_cc_box_rule: the parameters of unetpp_components_filter_box (all doubles)."""
    _fields_ = [(n, ctypes.c_double) for n in ("min_area", "max_area", "max_aspect", "min_side")]


class MorphElement(ctypes.Structure):
    """unetpp_morph_element: a structuring element in host memory, uint8 [kh,kw], anchor (ax, ay)."""
    _fields_ = [("kw", ctypes.c_int), ("kh", ctypes.c_int), ("ax", ctypes.c_int), ("ay", ctypes.c_int),
                ("host_data", ctypes.c_void_p)]


class MorphStep(ctypes.Structure):
    """unetpp_morph_step: P[dst] = op(P[a], P[b]) with elements[element], repeated `iterations` times."""
    _fields_ = [(n, ctypes.c_int) for n in ("op", "dst", "a", "b", "element", "iterations")]


class MergeStep(ctypes.Structure):
    """unetpp_merge_step: `op` with elements[element] on plane `plane`, `iterations` times."""
    _fields_ = [(n, ctypes.c_int) for n in ("plane", "op", "element", "iterations")]


class BilateralTables(ctypes.Structure):
    """unetpp_bilateral_tables: the weights and taps of the bilateral filter, all in host memory."""
    _fields_ = [("radius", ctypes.c_int32), ("n_taps", ctypes.c_int32), ("color_w", ctypes.POINTER(ctypes.c_float)),
                ("space_w", ctypes.POINTER(ctypes.c_float)), ("dy", ctypes.POINTER(ctypes.c_int32)), ("dx", ctypes.POINTER(ctypes.c_int32))]


ENHANCE_ALWAYS, ENHANCE_IF_GREY = 0, 1
MORPH_OPS = {"dilate": 0, "erode": 1, "and": 2, "andnot": 3, "or": 4, "copy": 5}
MERGE_OPS = {"dilate": 0, "erode": 1, "open": 6, "close": 7}                 # unetpp_merge_step.op
OVERLAY_MODES = {"region": 0, "weighted": 1}
DIST_METRICS = {"l1": 1, "l2": 2, "c": 3}          # UNETPP_DIST_*: cv2.DIST_L1, DIST_L2, DIST_C
RULES = {"argmax": 0, "thresholded_argmax": 1, "strict_bg_check": 2, "exclusive": 3}


class Outputs(ctypes.Structure):
    _fields_ = [("dev_logits", ctypes.c_void_p), ("dev_probs", ctypes.c_void_p), ("dev_mask", ctypes.c_void_p),
                ("dev_cable", ctypes.c_void_p), ("dev_tape", ctypes.c_void_p), ("rule", ctypes.c_int),
                ("t_cable", ctypes.c_float), ("t_tape", ctypes.c_float), ("bg_margin", ctypes.c_float),
                ("ct_margin", ctypes.c_float)]


vp, ci, cs, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double
i32p, f32p, u8p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
btp = ctypes.POINTER(BilateralTables)

# One table per public header, each holding every symbol that header declares: name -> (restype, argtypes).  BINDINGS below
# collects them and load() applies them.
ABI = {
    "unetpp_create": (ci, [ctypes.POINTER(Config), ctypes.POINTER(vp)]),
    "unetpp_destroy": (None, [vp]),
    "unetpp_last_error": (ctypes.c_char_p, [vp]),
    "unetpp_version": (ctypes.c_char_p, []),
    "unetpp_weights_blob_bytes": (cs, [ci, ci]),
    "unetpp_weights_blob_bytes_arch": (cs, [ci, ci, ci]),
    "unetpp_load_weights": (ci, [vp, vp, cs]),
    "unetpp_load_weights_device": (ci, [vp, vp, cs, vp]),
    "unetpp_forward": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]),
    "unetpp_forward_ex": (ci, [vp, vp, ci, ci, ci, ci, ctypes.POINTER(Outputs), vp]),
    "unetpp_mask_stats": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, vp]),
    "unetpp_resize_linear_u8": (ci, [vp, vp, ci, ci, ci, ci, vp, ci, ci, vp]),
    "unetpp_resize_nearest_roi_u8": (ci, [vp, vp, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, ci, vp]),
    "unetpp_workspace_bytes": (cs, [vp]),
    "unetpp_status": (ci, [vp, ctypes.POINTER(ctypes.c_uint32), ci]),
    "unetpp_profile_enable": (ci, [vp, ci]),
    "unetpp_profile_count": (ci, [vp]),
    "unetpp_profile_read": (ci, [vp, f32p, ci]),
    "unetpp_profile_name": (ctypes.c_char_p, [vp, ci]),
    "unetpp_profile_work": (ci, [vp, ci, ctypes.POINTER(cd), ctypes.POINTER(cd)]),
    "unetpp_profile_plan": (ci, [vp, ci, ctypes.POINTER(ci)]),
    "unetpp_debug_read": (ctypes.c_longlong, [vp, ctypes.c_char_p, f32p, cs]),
    "unetpp_debug_keep_intermediates": (ci, [vp, ci]),
    "unetpp_ds_blob_bytes": (cs, [ci]),
    "unetpp_load_ds_heads": (ci, [vp, vp, cs]),
    "unetpp_forward_ds": (ci, [vp, vp, ci, ci, ci, ci, ctypes.POINTER(ctypes.POINTER(Outputs)), vp]),
    "unetpp_components_workspace_bytes": (cs, [ci, ci, ci, ci]),
    "unetpp_components": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "unetpp_components_filter": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(CcRule), ctypes.c_uint8, vp, vp, vp]),
    "unetpp_morphology": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, ctypes.POINTER(MorphElement), ci, ctypes.POINTER(MorphStep), ci, ci,
                               ctypes.c_uint8, vp, vp]),
    "unetpp_morphology_layout": (ci, [ci, ci, ci, ctypes.POINTER(MorphElement), ci, ctypes.POINTER(MorphStep), ci,
                                      ctypes.POINTER(ci), ctypes.POINTER(ci)]),
    "unetpp_gray_u8": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "unetpp_gaussian_blur_u8": (ci, [vp, vp, ci, ci, ci, i32p, ci, vp, vp]),
    "unetpp_canny_workspace_bytes": (cs, [ci, ci, ci]),
    "unetpp_canny_layout": (ci, [ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]),
    "unetpp_canny_u8": (ci, [vp, vp, ci, ci, ci, i32p, ci, cd, cd, vp, vp, vp]),
    "unetpp_laplacian_band_u8": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, vp]),
    "unetpp_components_filter_box": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ctypes.POINTER(CcBoxRule), ctypes.c_uint8, vp, vp, vp]),
    "unetpp_edges_union_workspace_bytes": (cs, [ci]),
    "unetpp_edges_union_u8": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]),
    "unetpp_dog_band_u8": (ci, [vp, vp, vp, ci, ci, ci, i32p, ci, i32p, ci, ci, vp, vp]),
    "unetpp_count_nonzero_u8": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "unetpp_row_widths": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp]),
    "unetpp_width_profile": (ci, [vp, vp, ci, ci, f32p, ci, ci, vp, vp, vp, vp, vp]),
    "unetpp_components_summary": (ci, [vp, vp, vp, ci, ci, ctypes.c_int64, vp, vp]),
    "unetpp_tile_gather_u8": (ci, [vp, vp, ci, ci, ci, i32p, ci, i32p, ci, ci, ci, ci, vp, vp]),
    "unetpp_tile_gate_f32": (ci, [vp, vp, ci, ci, ci, ci, ctypes.c_float, vp, vp, vp]),
    "unetpp_tile_blend_f32": (ci, [vp, vp, ci, ci, ci, i32p, ci, i32p, ci, ci, vp, ci, ci, vp, vp, vp]),
    "unetpp_gray_decision": (ci, [vp, vp, ci, ci, ci, cd, vp, vp, vp]),
    "unetpp_clahe_u8": (ci, [vp, vp, ci, ci, ci, cd, ci, ci, vp, vp, vp, vp]),
    "unetpp_bilateral_u8": (ci, [vp, vp, ci, ci, ci, btp, vp, vp]),
    "unetpp_enhance_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, cd, cd, ci, ci, u8p, btp, vp, vp, vp, vp, vp]),
    "unetpp_enhance_workspace_bytes": (cs, [ci, ci, ci, ci, ci]),
    "unetpp_enhance_layout": (ci, [ctypes.POINTER(ci), ctypes.POINTER(ci)]),
    "unetpp_nlmeans_layout": (ci, [ctypes.POINTER(ci), ctypes.POINTER(ci)]),
    "unetpp_nlmeans_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, vp, vp]),
    "unetpp_evaluation_layout": (ci, [ctypes.POINTER(ci)]),
    "unetpp_confusion_u8": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]),
    "unetpp_mask_disagreement": (ci, [vp, vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp]),
    "unetpp_probmap_layout": (ci, [ctypes.POINTER(ci)]),
    "unetpp_prob_levels_f32": (ci, [vp, vp, ci, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp, vp]),
    "unetpp_prob_threshold_hist_f32": (ci, [vp, vp, ci, ci, vp, ci, ci, ci, f32p, ci, ci, ci, vp, vp, vp, vp]),
    "unetpp_components_prob_sum_f32": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "unetpp_components_filter_mean": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint8, vp, vp, vp]),
    "unetpp_distance_workspace_bytes": (cs, [ci, ci, ci]),
    "unetpp_distance_transform_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, ci, ctypes.c_float, ctypes.c_float, ctypes.c_uint8, vp, vp, vp]),
    "unetpp_components_best_cable": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, cd, ci, ci, cd, ctypes.c_uint8, vp, vp, vp]),
    "unetpp_roi_limit_workspace_bytes": (cs, [ci]),
    "unetpp_roi_limit_u8": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]),
    "unetpp_row_width_median": (ci, [vp, vp, ci, ci, vp, vp]),
    "unetpp_quality_gate_workspace_bytes": (cs, [ci]),
    "unetpp_quality_gate_u8": (ci, [vp, vp, vp, ci, ci, ci, ci, cd, cd, cd, cd, vp, vp, vp, vp, vp, vp, vp, vp]),
    "unetpp_threshold_classes_f32": (ci, [vp, vp, ctypes.c_int64, ci, ctypes.POINTER(ctypes.c_int64), ci, ci, ci, f32p, ctypes.c_float, ci, ci,
                                          vp, vp]),
    "unetpp_merge_classes": (ci, [vp, vp, ci, ci, ci, u8p, ci, i32p, ctypes.POINTER(MorphElement), ci, ctypes.POINTER(MergeStep), ci, vp, vp,
                                  ci, vp]),
    "unetpp_merge_classes_layout": (ci, [ci, ci, ci, ci, ctypes.POINTER(MorphElement), ci, ctypes.POINTER(MergeStep), ci,
                                         ctypes.POINTER(ci), ctypes.POINTER(ci)]),
    "unetpp_overlay_u8": (ci, [vp, vp, vp, ci, ci, ci, u8p, u8p, ctypes.c_float, ctypes.c_float, ci, vp, vp]),
}
ABI_SYMBOLS = list(ABI)


class RoiCcRule(ctypes.Structure):
    """unetpp_roi_cc_rule: the parameters of unetpp_roi_components_select (all doubles)."""
    _fields_ = [(n, ctypes.c_double) for n in ("min_area", "min_aspect", "wide_width", "edge_lo", "edge_hi", "large_area")]


ROI_RULES = {"geometry": 0, "primary": 1}

# include/unetpp_roi.h
ABI_ROI = {
    "unetpp_roi_projection_workspace_bytes": (cs, [ci, ci]),
    "unetpp_roi_stats_workspace_bytes": (cs, [ci]),
    "unetpp_roi_from_edges_u8": (ci, [vp, vp, ci, ci, ci, vp, vp, vp]),
    "unetpp_roi_crop_resize_u8": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, vp]),
    "unetpp_roi_adaptive_thresholds_f32": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]),
    "unetpp_roi_ultra_strict_f32": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp]),
    "unetpp_roi_components_select": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ctypes.POINTER(RoiCcRule), ctypes.c_uint8, vp, vp, vp]),
    "unetpp_roi_paste_masks_u8": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp, ci, ci, vp]),
}

# include/unetpp_loss.h
ABI_LOSS = {
    "unetpp_loss_layout": (ci, [ctypes.POINTER(ci)]),
    "unetpp_loss_sums_f32": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]),
}

# include/unetpp_contours.h
ABI_CONTOURS = {
    "unetpp_contours_workspace_bytes": (cs, [ci, ci, ci, ci]),
    "unetpp_contour_areas_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "unetpp_contour_circle": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]),
    "unetpp_paste_roi_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "unetpp_overlay_chain_u8": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, u8p, vp, vp]),
}

PIXEL_RULES = {"relative": 0, "confidence": 1}     # UNETPP_PIXEL_*

# include/unetpp_simple_loops.h
ABI_SIMPLE_LOOPS = {
    "unetpp_pixel_rules_f32": (ci, [vp, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp, vp, vp]),
    "unetpp_components_keep": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ctypes.c_uint8, vp, vp, vp]),
    "unetpp_tape_position_filter_u8": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp]),
    "unetpp_column_band_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp]),
    "unetpp_mask_join_u8": (ci, [vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, vp, vp]),
}

RAW_PATTERNS = {"BG": 0, "GB": 1, "RG": 2, "GR": 3, "MONO": 4}          # UNETPP_RAW_*

# include/unetpp_raw.h
ABI_RAW = {
    "unetpp_raw_to_bgr_u8": (ci, [vp, vp, ctypes.c_int64, ctypes.c_int64, ci, ci, ci, ci, vp, vp, vp]),
    "unetpp_raw_resize_u8": (ci, [vp, vp, ctypes.c_int64, ctypes.c_int64, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp]),
}

ROTATE_CODES = {"90_cw": 0, "180": 1, "90_ccw": 2}                      # UNETPP_ROTATE_*: cv2.ROTATE_90_CLOCKWISE, ROTATE_180, ROTATE_90_COUNTERCLOCKWISE

# include/unetpp_two_stage.h
ABI_TWO_STAGE = {
    "unetpp_two_stage_masks_u8": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "unetpp_two_stage_overlay_u8": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp]),
    "unetpp_rotate_u8": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp]),
}

# include/unetpp_loss_grad.h
ABI_LOSS_GRAD = {
    "unetpp_loss_grad_layout": (ci, [ctypes.POINTER(ci)]),
    "unetpp_loss_grad_f32": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]),
    "unetpp_loss_narrow_target_i64": (ci, [vp, vp, ctypes.c_int64, vp, vp]),
}

# include/unetpp_train_batch.h
ABI_TRAIN_BATCH = {
    "unetpp_train_batch_layout": (ci, [ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]),
    "unetpp_train_crop_rects": (ci, [vp, vp, ctypes.c_int64, vp, ci, vp, ci, vp, vp]),
    "unetpp_train_batch_u8": (ci, [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ci, vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, vp, vp, vp]),
}

# public header (a file of include/) -> its table; a new entry-point family adds its table above and one line here
BINDINGS = {"unetpp.h": ABI, "unetpp_roi.h": ABI_ROI, "unetpp_loss.h": ABI_LOSS, "unetpp_contours.h": ABI_CONTOURS,
            "unetpp_simple_loops.h": ABI_SIMPLE_LOOPS, "unetpp_raw.h": ABI_RAW, "unetpp_two_stage.h": ABI_TWO_STAGE,
            "unetpp_loss_grad.h": ABI_LOSS_GRAD, "unetpp_train_batch.h": ABI_TRAIN_BATCH}
_names = [n for table in BINDINGS.values() for n in table]
if len(set(_names)) != len(_names):
    raise ImportError(f"bound in two tables of BINDINGS: {sorted(n for n in set(_names) if _names.count(n) > 1)}")

# -fno-slp-vectorize: the SLP vectoriser turns pairs of float operations into v_pk_mul_f32 / v_pk_fma_f32, and a packed
# fp32 instruction issued beside another wave's MFMA stream on the same SIMD takes 26-58 cycles instead of 5-7
# (scripts/microbench/valu_beside_mfma.hip) -- the loader waves of the wave-specialised kernels run exactly there.
CXXFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize"]


def source_hash() -> str:
    """Digest of every file the library is compiled from and of the compiler flags; baked into the binary
    (unetpp_version() ends in 'src:<hash>') so that a .so built from other sources is recognised wherever it travels."""
    h = hashlib.sha256()
    h.update(" ".join(CXXFLAGS).encode() + b"\0")
    for rel in sorted(SOURCES + HEADERS):
        with open(os.path.join(CSRC, rel), "rb") as f:
            h.update(rel.encode() + b"\0" + f.read() + b"\0")
    return h.hexdigest()[:16]


def built_hash(path: str = LIB_PATH):
    """The 'src:' tag of a built library, read from the file (no dlopen), or None."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    i = blob.find(b"(gfx950) src:")
    if i < 0:
        return None
    tag = blob[i + 13:i + 13 + 16]
    if blob[i + 29:i + 36] == b" +wsdbg" and not os.environ.get("UNETPP_ALLOW_DBG_LIB"):
        return "wsdbg-build"                 # a measurement build never counts as current
    return tag.decode("ascii", "replace")


def _stale() -> bool:
    return built_hash() != source_hash()


def _hipcc():
    cand = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return cand if os.path.exists(cand) else shutil.which("hipcc")


def build(force: bool = False, verbose: bool = False, defines=()) -> str:
    """hipcc --offload-arch=gfx950 -> unet-_amd/libunetpp_hip.so (cross-compiles without a GPU).

    defines: extra preprocessor symbols ("NAME" or "NAME=VALUE") of a measurement build (scripts/ws_ablate.sh and its
    kin); such a build is always compiled.  With UNETPP_WS_DBG among them the library tags itself "+wsdbg" and does not
    count as the product build: built_hash() and load() refuse it unless UNETPP_ALLOW_DBG_LIB is set."""
    if not force and not defines and not _stale():
        return LIB_PATH
    hipcc = _hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found: cannot build libunetpp_hip.so")
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"      # several ranks may build at once: write aside, then rename atomically
    cmd = [hipcc] + CXXFLAGS + ["-shared", "-fPIC", f'-DUNETPP_SRC_HASH="{source_hash()}"'] + [f"-D{d}" for d in defines] + [
           "-o", tmp] + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd).replace(tmp, LIB_PATH), flush=True)
    try:
        subprocess.run(cmd, check=True, cwd=CSRC)
        os.replace(tmp, LIB_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return LIB_PATH


_lib = None


def share_torch_hip_runtime() -> None:
    """Import torch (when it is installed) BEFORE the library is dlopen'ed.  The torch wheel ships its own
    libamdhip64 / libhsa-runtime64; loaded first, they satisfy this library's DT_NEEDED entries and the process has
    one HIP runtime.  The other way round the library pulls in /opt/rocm's copies, torch adds its own, and whichever
    runtime initialises second finds no device ("no HIP device available" from unetpp_create after a torch CUDA call)."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load(build_if_missing: bool = True) -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    share_torch_hip_runtime()
    if _stale():
        # missing, or built from other sources than the tree holds (the .so is git-ignored but travels to the GPU
        # box): rebuild when a compiler is at hand, otherwise refuse -- never run kernels that do not match the tree
        what = "is missing" if not os.path.exists(LIB_PATH) else f"was built from other sources (src:{built_hash()}, tree {source_hash()})"
        if not build_if_missing or not _hipcc():
            raise RuntimeError(f"{LIB_PATH} {what}: build it with __graft_entry__.build(); there is no CPU fallback")
        build()
    lib = ctypes.CDLL(LIB_PATH)
    for table in BINDINGS.values():
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    ver = lib.unetpp_version().decode()
    if ver.endswith(" +wsdbg") and os.environ.get("UNETPP_ALLOW_DBG_LIB"):
        ver = ver[:-len(" +wsdbg")]            # measurement build with phase ablations (scripts/ws_ablate.sh)
    if not ver.endswith("src:" + source_hash()):
        raise RuntimeError(f"{LIB_PATH} reports {lib.unetpp_version().decode()!r}, tree is src:{source_hash()}")
    _lib = lib
    return lib
