"""The Python surface that callers and the other files of the package rely on, pinned without a device: the public methods
of NestedUNet / SimpleUNet and their signatures, the private names used outside nested_unet.py and postproc.py, and
the text each method's tensor check raises for a host tensor."""
import inspect

import pytest

# str(inspect.signature(NestedUNet.<name>)) of every public method, as the methods stood before postproc.py was split off
SIGNATURES = {
    'analyze_defects': ("(self, pred, cable_cls: 'int' = 1, tape_cls: 'int' = 2, defect_classes=(3, 4, 5, 6), hole_min_size: 'int' = 10, "
        "max_components: 'int' = 8192, check: 'bool' = True)"),
    'bgr_to_gray': '(self, frames)',
    'bilateral_filter': "(self, gray, d: 'int' = 5, sigma_color: 'float' = 75.0, sigma_space: 'float' = 75.0, tables=None)",
    'blend_tiles': "(self, maps, frame_hw, patch_size: 'int' = 384, stride: 'int' = 192, include=None, return_output: 'bool' = True)",
    'boundary_band': "(self, mask_cable, match_class: 'int' = -1, band_out: 'int' = 10, out_value: 'int' = 255)",
    'burr_mask_dog': ("(self, gray, mask_cable, match_class: 'int' = -1, *, band_out: 'int' = 10, threshold=30, min_area=20, max_area=500, "
        "taps1=None, taps2=None, out_value: 'int' = 255, max_components: 'int' = 8192, check: 'bool' = True)"),
    'burr_mask_rulebased': ("(self, gray, mask_cable, match_class: 'int' = -1, *, band_out: 'int' = 10, laplacian_threshold=30, min_area=20, "
        "max_area=500, out_value: 'int' = 255, max_components: 'int' = 8192, check: 'bool' = True)"),
    'burrs_from_edges': ("(self, edges, mask_cable, match_class: 'int' = -1, *, min_area=30, max_area=800, band_ksize: 'int' = 8, close_ksize: "
        "'int' = 3, open_ksize: 'int' = 2, max_aspect=5.0, min_side=3, out_value: 'int' = 1, max_components: 'int' = 8192, "
        "check: 'bool' = True)"),
    'canny': '(self, gray, low, high, blur=None)',
    'clahe': "(self, gray, clip_limit: 'float' = 2.0, tile_grid=(8, 8), return_luts: 'bool' = False)",
    'components': "(self, mask, match_class: 'int' = -1, connectivity: 'int' = 8, max_components: 'int' = 8192)",
    'components_summary': "(self, num, stats, min_area: 'int' = 0)",
    'constrain_tape_to_ring': ("(self, mask_tape, mask_cable, tape_class: 'int' = -1, cable_class: 'int' = -1, ring_dilate: 'int' = 15, ring_erode: "
        "'int' = 5, out_value: 'int' = 255, max_components: 'int' = 8192, check: 'bool' = True)"),
    'count_nonzero': '(self, mask)',
    'cuda': '(self, device=None)',
    'debug_activation': "(self, name: 'str', b: 'int', h: 'int', w: 'int') -> 'np.ndarray'",
    'debug_keep_intermediates': "(self, on: 'bool' = True)",
    'detect_burrs': ("(self, gray, mask_cable, match_class: 'int' = -1, *, min_area=30, max_area=800, band_ksize: 'int' = 8, blur_ksize: "
        "'int' = 5, blur_sigma: 'float' = 1.0, taps=None, canny_low=50, canny_high=150, close_ksize: 'int' = 3, open_ksize: "
        "'int' = 2, max_aspect=5.0, min_side=3, out_value: 'int' = 1, max_components: 'int' = 8192, check: 'bool' = True)"),
    'detect_burrs_enhanced': ("(self, gray, mask_cable, match_class: 'int' = -1, *, min_area=50, max_area=500, band_ksize: 'int' = 25, blur_ksize: "
        "'int' = 5, blur_sigma: 'float' = 1.0, taps=None, canny_low=30, canny_high=100, sobel_threshold=50, "
        "laplacian_threshold=15, close_ksize: 'int' = 5, open_ksize: 'int' = 3, max_aspect=6.0, min_side=4, out_value: 'int' = "
        "1, max_components: 'int' = 8192, check: 'bool' = True)"),
    'diameter_metrics': ("(self, pred, cable_cls: 'int' = 1, tape_cls: 'int' = 2, mm_per_px: 'float' = 0.05, min_valid_rows: 'int' = 20, "
        "kernel_size: 'int' = 31, min_area=50, taps=None, max_components: 'int' = 8192, check: 'bool' = True)"),
    'diameter_profile': ("(self, pred, cable_cls: 'int', wrap_cls: 'int', kernel_size: 'int' = 31, taps=None, max_components: 'int' = 8192, "
        "check: 'bool' = True)"),
    'dog_band': '(self, gray, band, *, threshold=30, taps1=None, taps2=None)',
    'edges_combined': ('(self, gray, canny_edges=None, *, blur=(5, 1.0), canny_low=30, canny_high=100, sobel_threshold=50, '
        'laplacian_threshold=15)'),
    'enhance_grayscale': ("(self, frames, *, clip_limit: 'float' = 2.0, tile_grid=8, gamma: 'float' = 0.8, denoise_method: 'str' = 'bilateral', "
        "denoise_strength: 'int' = 5, channels_out: 'int' = 3)"),
    'eval': '(self)',
    'filter_components': ("(self, mask, match_class: 'int' = -1, rule: 'str' = 'largest', *, connectivity: 'int' = 8, max_components: 'int' = "
        "8192, out_value: 'int' = 1, check: 'bool' = True, min_area=None, min_width=50, max_width=300, min_height_ratio=0.3, "
        'min_aspect=1.6, max_center_offset=0.3, roi_width=None)'),
    'filter_components_box': ("(self, mask, match_class: 'int' = -1, min_area=30, max_area=800, max_aspect=inf, min_side=0, *, connectivity: 'int' = "
        "8, max_components: 'int' = 8192, out_value: 'int' = 1, check: 'bool' = True)"),
    'forward': "(self, x, output: 'int' = 0)",
    'forward_deep_supervision': '(self, x)',
    'gather_tiles': "(self, frames, patch_size: 'int' = 384, stride: 'int' = 192, target_size: 'int' = 256, channel_order: 'str' = 'rgb')",
    'gaussian_blur': "(self, gray, ksize: 'int' = 5, sigma: 'float' = 1.0, taps=None)",
    'has_burr': '(self, mask, min_total_area=50)',
    'is_grayscale': "(self, frames, threshold: 'float' = 10.0, return_sums: 'bool' = False)",
    'load_state_dict': "(self, state_dict, strict: 'bool' = True)",
    'load_weights_from_device_blob': '(self, blob_tensor)',
    'mask_stats': '(self, mask)',
    'morphology': ("(self, mask, match_class: 'int' = -1, op: 'str' = 'close', ksize=5, shape: 'str' = 'ellipse', iterations: 'int' = 1, "
        "element=None, anchor=None, out_value: 'int' = 1)"),
    'morphology_cleanup': "(self, mask, match_class: 'int' = -1, kernel_size: 'int' = 3, out_value: 'int' = 1)",
    'morphology_program': "(self, mask0, match0, steps, elements, mask1=None, match1: 'int' = -1, result_plane: 'int' = 2, out_value: 'int' = 1)",
    'postprocess_masks': ("(self, pred, cable_class: 'int' = 1, tape_class: 'int' = 2, roi_width=None, *, min_area=1000, min_aspect=1.6, "
        "max_center_offset=0.3, ring_dilate: 'int' = 15, ring_erode: 'int' = 5, out_value: 'int' = 255, max_components: 'int' ="
        " 8192, check: 'bool' = True)"),
    'predict_proba': "(self, x, output: 'int' = 0)",
    'predict_tiled': ("(self, frames, patch_size: 'int' = 384, stride: 'int' = 192, target_size: 'int' = 256, blend: 'str' = 'logits', "
        "gate_thr=None, gate_class: 'int' = 1, channel_order: 'str' = 'rgb', return_output: 'bool' = True)"),
    'preprocess_frames': ("(self, frames, enable: 'bool' = True, threshold: 'float' = 10.0, *, clip_limit: 'float' = 2.0, tile_grid=8, gamma: "
        "'float' = 0.8, denoise_method: 'str' = 'bilateral', denoise_strength: 'int' = 5, return_decisions: 'bool' = False)"),
    'profile': "(self, on: 'bool' = True)",
    'profile_plan': '(self)',
    'profile_read': '(self)',
    'raise_on_range_error': '(self)',
    'resize_frames': '(self, frames, size_hw)',
    'resize_masks': "(self, pred, frame_size_wh, match_class: 'int' = -1, roi=None)",
    'row_widths': "(self, mask0, match0: 'int' = -1, mask1=None, match1: 'int' = -1)",
    'segment': "(self, x, return_logits: 'bool' = False, return_class_masks: 'bool' = False, output: 'int' = 0)",
    'segment_thresholded': ("(self, x, rule: 'str' = 'thresholded_argmax', t_cable: 'float' = 0.45, t_tape: 'float' = 0.5, bg_margin: 'float' = "
        "0.15, ct_margin: 'float' = 0.1, return_probs: 'bool' = False, output: 'int' = 0)"),
    'state_dict': '(self)',
    'status': "(self, clear: 'bool' = False) -> 'int'",
    'tape_holes': "(self, pred, tape_class: 'int' = 2, hole_min_size: 'int' = 10, max_components: 'int' = 8192, check: 'bool' = True)",
    'thickness_profile': "(self, pred, cable_cls: 'int' = 1, tape_cls: 'int' = 2, mm_per_px: 'float' = 0.05, kernel_size: 'int' = 31, taps=None)",
    'tile_gate': "(self, maps, gate_thr, gate_class: 'int' = 1)",
    'to': '(self, device)',
    'train': "(self, mode: 'bool' = True)",
    'width_profile': "(self, widths, kernel_size: 'int' = 31, min_valid_rows: 'int' = 20, taps=None, want_delta: 'bool' = True)",
    'workspace_bytes': "(self) -> 'int'",
}

PRIVATE = ("_ensure_engine", "_handle", "_device_index", "_components", "_morph_named", "_morph_launch", "_diameter_metrics",
           "_analyze_defects", "_check_and_build_blob", "_ds_blob", "_ds_uploaded", "_cc_workspaces", "_morph_programs",
           "_SIZE_MULTIPLE", "_ARCH")


def public(cls):
    return sorted(n for n in dir(cls) if not n.startswith("_") and callable(getattr(cls, n)))


def test_public_methods_and_signatures_are_unchanged():
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    assert len(SIGNATURES) == 61
    assert {n: str(inspect.signature(getattr(NestedUNet, n))) for n in public(NestedUNet)} == SIGNATURES
    assert public(SimpleUNet) == sorted(SIGNATURES)


def test_private_names_other_files_use_exist():
    from unet_amd.nested_unet import NestedUNet, SimpleUNet
    for model in (NestedUNet(3), SimpleUNet(3)):
        assert [n for n in PRIVATE if not hasattr(model, n)] == []


@pytest.mark.parametrize("cls", ["NestedUNet", "SimpleUNet"])
@pytest.mark.parametrize("C", [0, 9, -1])
def test_a_class_count_outside_1_to_8_is_refused_with_the_engines_message(C, cls):
    """unetpp_create checks num_classes before it touches a device: the heads keep 8 class slots in registers"""
    from unet_amd import nested_unet
    model = getattr(nested_unet, cls)(C).to("cuda:0")
    with pytest.raises(RuntimeError) as err:
        model._ensure_engine(1, 16, 16)
    assert str(err.value) == f"unetpp_create failed (-1): num_classes={C} out of range [1,8]"
    assert model._handle is None


# ---- the tensor check: (text after the tensor's name, which host tensor, the methods, extra positional arguments) ------
MASK, FRAMES, WIDTHS, MAPS, NUM = "mask", "frames", "widths", "maps", "num"
TWO = ("constrain_tape_to_ring", "burrs_from_edges", "burr_mask_dog", "detect_burrs", "burr_mask_rulebased", "detect_burrs_enhanced",
       "dog_band")                                                               # these take two images: the same one twice
EXTRA = {"gather_tiles": (16, 8, 16), "predict_tiled": (16, 8, 16), "blend_tiles": ((16, 16), 16, 8), "resize_frames": ((8, 8),),
         "resize_masks": ((8, 8),), "canny": (50, 150), "diameter_profile": (1, 2), "components_summary": (None,), "tile_gate": (0.5,)}
MESSAGES = [
    ("mask must be a uint8 CUDA tensor [B,H,W]", MASK,
     ["mask_stats", "components", "filter_components", "filter_components_box", "morphology", "morphology_cleanup", "boundary_band",
      "constrain_tape_to_ring", "postprocess_masks", "tape_holes", "burrs_from_edges", "burr_mask_dog", "count_nonzero", "has_burr"]),
    ("mask0 must be a uint8 CUDA tensor [B,H,W]", MASK, ["row_widths"]),
    ("pred must be a uint8 CUDA tensor [B,H,W]", MASK,
     ["diameter_metrics", "thickness_profile", "diameter_profile", "analyze_defects", "resize_masks"]),
    ("gray must be a uint8 CUDA tensor [B,H,W]", MASK,
     ["gaussian_blur", "canny", "detect_burrs", "burr_mask_rulebased", "edges_combined", "detect_burrs_enhanced", "dog_band", "clahe",
      "bilateral_filter"]),
    ("frames must be a uint8 CUDA tensor [B,H,W,3]", FRAMES, ["bgr_to_gray", "gather_tiles", "predict_tiled"]),
    ("frames must be a uint8 CUDA tensor [B,H,W,3] or [B,H,W]", FRAMES, ["is_grayscale", "enhance_grayscale", "preprocess_frames"]),
    ("frames must be a uint8 CUDA tensor [B,H,W,C]", FRAMES, ["resize_frames"]),
    ("widths must be a float32 CUDA tensor [B,2,H]", WIDTHS, ["width_profile"]),
    ("num must be an int32 CUDA tensor [B]", NUM, ["components_summary"]),
    ("maps must be a float32 CUDA tensor [N,C,T,T]", MAPS, ["tile_gate", "blend_tiles"]),
    ("input must be a CUDA (HIP) tensor on the engine's device", MAPS, ["forward", "segment"]),
]
CASES = [(text, kind, name) for text, kind, names in MESSAGES for name in names]


@pytest.fixture(scope="module")
def host_tensors():
    import torch
    return {MASK: torch.zeros((1, 16, 16), dtype=torch.uint8), FRAMES: torch.zeros((1, 16, 16, 3), dtype=torch.uint8),
            WIDTHS: torch.zeros((1, 2, 16), dtype=torch.float32), MAPS: torch.zeros((1, 3, 16, 16), dtype=torch.float32),
            NUM: torch.zeros((1,), dtype=torch.int32)}


@pytest.mark.parametrize("cls", ["NestedUNet", "SimpleUNet"])
@pytest.mark.parametrize("text,kind,name", CASES, ids=[c[2] for c in CASES])
def test_a_host_tensor_is_refused_with_the_methods_message(text, kind, name, cls, host_tensors):
    from unet_amd import nested_unet
    model = getattr(nested_unet, cls)(3)
    t = host_tensors[kind]
    with pytest.raises(RuntimeError) as err:
        getattr(model, name)(*((t, t) if name in TWO else (t,)), *EXTRA.get(name, ()))
    assert str(err.value) == text
    assert model._handle is None
