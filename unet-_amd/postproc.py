"""The post-processing methods of ``NestedUNet`` and ``SimpleUNet``: everything the frame loops do with masks and frames
around the network, on the device, behind the entry points of csrc/unetpp_postproc.hip.  The NumPy forms and the
argument checks are in components.py, morphology.py, edges.py, enhance.py, geometry.py and tiling.py."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


class PostProcessing:
    """Mixin of NestedUNet (nested_unet.py), which owns the engine: _handle, _device_index, _ensure_engine, _prepare, _err."""

    # ------------------------------------------------------------------ what every method below shares
    def _input(self, t, what="gray", shape="[B,H,W]", dtype="uint8"):
        """A contiguous `dtype` CUDA tensor of `shape` on the engine's device, with the engine made ready.  `shape` is the
        text of the message and the check: a number fixes that size, a repeated letter makes two sizes equal, ' or '
        separates alternatives."""
        import torch

        def fits(dims):
            return t.dim() == len(dims) and all(t.shape[i] == (int(d) if d.isdigit() else t.shape[dims.index(d)])
                                                for i, d in enumerate(dims))
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, dtype) and
                any(fits(alt.strip("[]").split(",")) for alt in shape.split(" or "))):
            raise RuntimeError(f"{what} must be {'an' if dtype[0] == 'i' else 'a'} {dtype} CUDA tensor {shape}")
        if self._device_index is None:
            self.to(t.device)
        if t.device.index != self._device_index:
            raise RuntimeError(f"{what} on {t.device}, engine on cuda:{self._device_index}")
        self._ensure_engine(1, self._SIZE_MULTIPLE, self._SIZE_MULTIPLE)
        return t.contiguous()

    def _call(self, name, *args, stream_of, invalid=ValueError):
        """lib.<name>(handle, *args, stream) for a launching entry of include/unetpp.h: tensors go as their device
        pointers, the stream is the current one of stream_of's device (returned, in its ctypes form).  A non-zero code
        raises RuntimeError, or `invalid` for -2 (an argument the kernel does not support)."""
        import torch
        args = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        stream = ctypes.c_void_p(torch.cuda.current_stream(stream_of.device).cuda_stream)
        rc = getattr(_lib.load(), name)(self._handle, *args, stream)
        if rc != 0:
            raise (invalid if rc == -2 else RuntimeError)(self._err(rc))
        return stream

    def _workspace(self, key, nbytes, device, unsupported):
        """The scratch buffer kept under `key` in _cc_workspaces; on a miss nbytes() asks the library for its size, and
        0 bytes is RuntimeError(unsupported) unless that is None."""
        import torch
        ws = self._cc_workspaces.get(key)
        if ws is None or ws.device != device:
            n = int(nbytes())
            if n == 0 and unsupported is not None:
                raise RuntimeError(unsupported)
            ws = self._cc_workspaces[key] = torch.empty(n, dtype=torch.uint8, device=device)
        return ws

    @staticmethod
    def _raise_overflow(over, k, what):
        """`over` bool [B] on the device (one read-back, synchronises): the frames whose labelling overflowed."""
        bad = over.nonzero().flatten().cpu().tolist()
        if bad:
            raise RuntimeError(f"{what}: frame {bad[0]} has more than max_components - 1 = {k - 1} components in one of its "
                               f"labellings: raise max_components")

    @staticmethod
    def _raise_num_overflow(num, k):
        """`num` int32 [B] of _components (one read-back, synchronises): the frames with more labels than the k rows."""
        for i, v in enumerate(num.cpu().tolist()):
            if v > k:
                raise RuntimeError(f"filter_components: frame {i} has num = {v} labels (background included), more than "
                                   f"max_components = {k}: raise max_components")

    # ------------------------------------------------------------------ mask statistics
    def mask_stats(self, mask):
        """Device-side reductions of a uint8 class-index mask [B,H,W] (e.g. from segment()):
        returns (counts int64 [B,C], widths float32 [B,C,H]) where counts[b,c] = np.sum(mask[b]==c)
        (infer_two_stage_burr.py:333-334) and widths[b,c,y] = xs.max()-xs.min()+1 over the columns of class c
        in row y, 0 for empty rows (_compute_width_per_row, src/utils/geometry_enhanced.py:45-74, before its
        optional smoothing).  Only B*C*(2H+1) integers cross to the caller instead of the mask."""
        import torch
        mask = self._input(mask, "mask")
        b, h, w = mask.shape
        c = self.num_classes
        counts = torch.empty((b, c), dtype=torch.int32, device=mask.device)
        rmin = torch.empty((b, c, h), dtype=torch.int32, device=mask.device)
        rmax = torch.empty((b, c, h), dtype=torch.int32, device=mask.device)
        self._call("unetpp_mask_stats", mask, b, h, w, counts, rmin, rmax, stream_of=mask, invalid=RuntimeError)
        widths = torch.where(rmax >= 0, (rmax - rmin + 1), torch.zeros_like(rmax)).to(torch.float32)
        return counts.to(torch.int64), widths

    # ------------------------------------------------------------------ connected components
    def _components(self, mask, match_class, connectivity, max_components, want_stats: bool):
        import torch
        mask = self._input(mask, "mask")
        if connectivity not in (4, 8):
            raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
        k = int(max_components)
        if k < 2:
            raise ValueError(f"max_components must be at least 2 (background + one component), got {max_components!r}")
        b, h, w = mask.shape
        dev = mask.device
        ws = self._workspace((b, h, w, k), lambda: _lib.load().unetpp_components_workspace_bytes(b, h, w, k), dev,
                             f"components: unsupported shape {tuple(mask.shape)}")
        labels = torch.empty((b, h, w), dtype=torch.int32, device=dev)
        num = torch.empty((b,), dtype=torch.int32, device=dev)
        stats = torch.empty((b, k, 5), dtype=torch.int32, device=dev) if want_stats else None
        sums = torch.empty((b, k, 2), dtype=torch.int64, device=dev) if want_stats else None   # uint64 bits; values < 2^63
        stream = self._call("unetpp_components", mask, b, h, w, int(match_class), int(connectivity), k, labels, num, stats, sums, ws,
                            stream_of=mask, invalid=RuntimeError)
        return labels, num, stats, sums, ws, stream

    def components(self, mask, match_class: int = -1, connectivity: int = 8, max_components: int = 8192):
        """cv2.connectedComponentsWithStats(mask == match_class, connectivity) on the device for a uint8 CUDA mask
        [B,H,W] (any H, W; match_class < 0: mask != 0).  Returns (labels int32 [B,H,W], num int32 [B],
        stats int32 [B,K,5], centroids float64 [B,K,2]) with K = max_components rows: stats in cv2's column order
        LEFT, TOP, WIDTH, HEIGHT, AREA, row 0 = background, rows >= num zero (centroids NaN there); num counts the
        background like cv2's num_labels and is exact even beyond K.  Labels are numbered in raster order of each
        component's first pixel (scipy.ndimage.label's order, not cv2's, which only matters for ties)."""
        import torch
        labels, num, stats, sums, _, _ = self._components(mask, match_class, connectivity, max_components, True)
        centroids = sums.to(torch.float64) / stats[:, :, 4:5].to(torch.float64)
        return labels, num, stats, centroids

    def filter_components(self, mask, match_class: int = -1, rule: str = "largest", *, connectivity: int = 8,
                          max_components: int = 8192, out_value: int = 1, check: bool = True, min_area=None,
                          min_width=50, max_width=300, min_height_ratio=0.3, min_aspect=1.6, max_center_offset=0.3,
                          roi_width=None):
        """The reference's component filters on the device: uint8 [B,H,W], out_value where the pixel's component is kept.
        rule='largest'      _largest_connected_component(mask, min_area=100), src/utils/geometry_enhanced.py:81-110;
                            min_area=0 is the tail of constrain_tape_to_ring (src/refactor/postprocess.py:106-116)
        rule='spatial'      spatial_filter(mask, min_width, max_width, min_height_ratio), infer_video_spatial.py:24-53
                            (min_area=1000, fixed in the reference)
        rule='cable_shape'  filter_cable_by_shape with PostprocessConfig's min_area=1000, min_aspect, max_center_offset
                            and roi_width (default W), src/refactor/postprocess.py:12-76; the reference's out_value is 255
        Ties between equal areas / scores go to the lower label (raster order of first pixels).  A frame with more than
        max_components - 1 components cannot be filtered: with check=True (one B-int read-back, synchronises) that
        raises RuntimeError, with check=False its output is all zero."""
        if rule not in _lib.CC_RULES:
            raise ValueError(f"rule must be one of {sorted(_lib.CC_RULES)}")
        out_value = self._check_out_value(out_value)
        import torch
        labels, num, stats, sums, ws, _ = self._components(mask, match_class, connectivity, max_components, True)
        b, h, w = labels.shape
        k = int(max_components)
        if min_area is None:
            min_area = 100 if rule == "largest" else 1000
        if roi_width is None:
            roi_width = w
        if rule == "cable_shape" and not float(roi_width) > 0:
            raise ValueError(f"roi_width must be positive, got {roi_width!r}")
        params = _lib.CcRule(float(min_area), float(min_width), float(max_width), float(min_height_ratio), float(min_aspect),
                             float(max_center_offset), float(roi_width))
        out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
        self._call("unetpp_components_filter", labels, num, stats, sums, b, h, w, k, _lib.CC_RULES[rule], ctypes.byref(params),
                   out_value, out, ws, stream_of=labels, invalid=RuntimeError)
        if check:
            self._raise_num_overflow(num, k)
        return out

    # ------------------------------------------------------------------ binary morphology
    @staticmethod
    def _check_out_value(out_value):
        if isinstance(out_value, bool) or not isinstance(out_value, (int, np.integer)) or not 1 <= int(out_value) <= 255:
            raise ValueError(f"out_value must be an integer in 1..255, got {out_value!r}")
        return int(out_value)

    def _morph_compile(self, key, elements, steps, result_plane):
        """The ctypes form of a checked program; cached under `key` (None: not cached).  The element arrays stay
        referenced from the entry: the C structures point into them."""
        if key is not None and key in self._morph_programs:
            return self._morph_programs[key]
        from . import morphology as mo
        elements, steps = mo.check_program(elements, steps, result_plane)
        c_el = (_lib.MorphElement * max(len(elements), 1))()
        for i, (arr, (ax, ay)) in enumerate(elements):
            c_el[i] = _lib.MorphElement(arr.shape[1], arr.shape[0], ax, ay, arr.ctypes.data)
        c_st = (_lib.MorphStep * max(len(steps), 1))()
        for i, st in enumerate(steps):
            c_st[i] = _lib.MorphStep(*st)
        entry = (elements, c_el, len(elements), c_st, len(steps), int(result_plane))
        if key is not None:
            self._morph_programs[key] = entry
        return entry

    def _morph_launch(self, compiled, mask0, match0, mask1, match1, out_value):
        import torch
        mask0 = self._input(mask0, "mask")
        if mask1 is not None:
            mask1 = self._input(mask1, "mask")
            if mask1.shape != mask0.shape:
                raise RuntimeError(f"mask1 {tuple(mask1.shape)} on {mask1.device} does not match mask0 {tuple(mask0.shape)} on {mask0.device}")
        b, h, w = mask0.shape
        _, c_el, n_el, c_st, n_st, result = compiled
        out = torch.empty((b, h, w), dtype=torch.uint8, device=mask0.device)
        self._call("unetpp_morphology", mask0, int(match0), mask1, int(match1), b, h, w, c_el, n_el, c_st, n_st, result, out_value, out,
                   stream_of=mask0)
        return out

    def morphology_program(self, mask0, match0, steps, elements, mask1=None, match1: int = -1, result_plane: int = 2,
                           out_value: int = 1):
        """One launch of a morphology program (include/unetpp.h, unetpp_morphology) on uint8 CUDA masks [B,H,W]: planes
        P0 = (mask0 == match0), P1 = (mask1 == match1) (match < 0: != 0; all zero without mask1), P2 / P3 scratch; steps
        are (op, dst, a, b, element, iterations) with op in dilate | erode | and | andnot | or | copy; elements are uint8
        arrays [kh,kw] or (array, (ax, ay)).  Returns uint8 [B,H,W] = out_value where P[result_plane] is set.  The
        semantics are cv2's (element not reflected, outside pixels never contribute); see unet_amd/morphology.py.
        ValueError for what the kernel does not support (element above 63, not row-convex, reach above 126)."""
        out_value = self._check_out_value(out_value)
        return self._morph_launch(self._morph_compile(None, elements, steps, result_plane), mask0, match0, mask1, match1, out_value)

    def morphology(self, mask, match_class: int = -1, op: str = "close", ksize=5, shape: str = "ellipse", iterations: int = 1,
                   element=None, anchor=None, out_value: int = 1):
        """cv2.dilate / cv2.erode / cv2.morphologyEx(MORPH_OPEN | MORPH_CLOSE) of (mask == match_class) with
        getStructuringElement(shape, ksize) (restated, unet_amd/morphology.py) or a caller-supplied `element` (e.g.
        cv2's own kernel) and `anchor` (ax, ay); open / close are one launch.  uint8 [B,H,W], out_value where set."""
        from . import morphology as mo
        out_value = self._check_out_value(out_value)
        if element is None:
            key = ("single", op, shape, ksize if isinstance(ksize, (int, np.integer)) else tuple(ksize), anchor if anchor is None else tuple(anchor),
                   int(iterations))
            if key not in self._morph_programs:
                self._morph_compile(key, *mo.program_single(op, mo.structuring_element(shape, ksize), anchor, int(iterations)))
            compiled = self._morph_programs[key]
        else:
            compiled = self._morph_compile(None, *mo.program_single(op, element, anchor, int(iterations)))
        return self._morph_launch(compiled, mask, match_class, None, -1, out_value)

    def _morph_named(self, name, params, builder):
        key = (name,) + tuple(params)
        if key not in self._morph_programs:
            self._morph_compile(key, *builder(*params))
        return self._morph_programs[key]

    def morphology_cleanup(self, mask, match_class: int = -1, kernel_size: int = 3, out_value: int = 1):
        """apply_morphology_cleanup (src/refactor/postprocess.py:144-166): open then close with ELLIPSE (k, k), one launch."""
        from . import morphology as mo
        out_value = self._check_out_value(out_value)
        return self._morph_launch(self._morph_named("cleanup", (int(kernel_size),), mo.program_cleanup), mask, match_class, None, -1, out_value)

    def boundary_band(self, mask_cable, match_class: int = -1, band_out: int = 10, out_value: int = 255):
        """The outer band of src/refactor/burr_detector.py:37-41: dilate(cable, ELLIPSE (2 band_out + 1)) - cable, one launch."""
        from . import morphology as mo
        out_value = self._check_out_value(out_value)
        return self._morph_launch(self._morph_named("band", (int(band_out),), mo.program_band), mask_cable, match_class, None, -1, out_value)

    def constrain_tape_to_ring(self, mask_tape, mask_cable, tape_class: int = -1, cable_class: int = -1, ring_dilate: int = 15,
                               ring_erode: int = 5, out_value: int = 255, max_components: int = 8192, check: bool = True):
        """constrain_tape_to_ring (src/refactor/postprocess.py:79-118): tape & (dilate(cable, E15) - erode(cable, E5)) in one
        morphology launch, then its largest component (filter_components, rule='largest', min_area=0)."""
        from . import morphology as mo
        out_value = self._check_out_value(out_value)
        ring = self._morph_launch(self._morph_named("ring", (int(ring_dilate), int(ring_erode)), mo.program_ring), mask_tape, tape_class,
                                  mask_cable, cable_class, 1)
        return self.filter_components(ring, 1, rule="largest", min_area=0, out_value=out_value, max_components=max_components, check=check)

    def postprocess_masks(self, pred, cable_class: int = 1, tape_class: int = 2, roi_width=None, *, min_area=1000, min_aspect=1.6,
                          max_center_offset=0.3, ring_dilate: int = 15, ring_erode: int = 5, out_value: int = 255,
                          max_components: int = 8192, check: bool = True):
        """postprocess_masks (src/refactor/postprocess.py:121-141, PostprocessConfig defaults) on a class mask [B,H,W]:
        (filter_cable_by_shape(pred == cable_class), constrain_tape_to_ring(pred == tape_class, filtered cable)), both
        uint8 [B,H,W] with out_value (255 in the reference), nothing leaving the device."""
        cable = self.filter_components(pred, cable_class, rule="cable_shape", min_area=min_area, min_aspect=min_aspect,
                                       max_center_offset=max_center_offset, roi_width=roi_width, out_value=out_value,
                                       max_components=max_components, check=check)
        tape = self.constrain_tape_to_ring(pred, cable, tape_class, -1, ring_dilate, ring_erode, out_value, max_components, check)
        return cable, tape

    def tape_holes(self, pred, tape_class: int = 2, hole_min_size: int = 10, max_components: int = 8192, check: bool = True):
        """The hole statistics of analyze_defects (src/utils/geometry_enhanced.py:281-295): holes = close(tape, ELLIPSE (5,5))
        - tape (one morphology launch), then the components with area >= hole_min_size.  Returns (tape_num_holes,
        hole area) as int64 [B] on the device, reduced there from the components' stats.  A frame with more than
        max_components - 1 hole components cannot be counted: with check=True (one B-int read-back, synchronises) that
        raises RuntimeError as filter_components does, with check=False its counts cover the first max_components - 1."""
        import torch
        from . import morphology as mo
        holes = self._morph_launch(self._morph_named("holes", (), mo.program_holes), pred, tape_class, None, -1, 1)
        k = int(max_components)
        _, num, stats, _, _, _ = self._components(holes, -1, 8, k, True)
        area = stats[:, 1:, 4].to(torch.int64)
        valid = area >= int(hole_min_size)
        num_holes, hole_area = valid.sum(1), (area * valid).sum(1)
        if check:
            self._raise_num_overflow(num, k)
        return num_holes, hole_area

    # ------------------------------------------------------------------ measurements (unet_amd/geometry.py is the NumPy form)
    def row_widths(self, mask0, match0: int = -1, mask1=None, match1: int = -1):
        """_compute_width_per_row(smooth=False) (src/utils/geometry_enhanced.py:61-67) of two binary planes of uint8
        CUDA masks [B,H,W] in one launch: plane 0 = (mask0 == match0), plane 1 = (mask1 == match1) (match < 0: != 0;
        mask1 may be mask0 itself, or None for an empty plane 1).  Returns (widths float32 [B,2,H] = last - first + 1
        over the foreground columns of a row, 0 for an empty row; area int64 [B,2] = foreground pixels)."""
        import torch
        mask0 = self._input(mask0, "mask0")
        if mask1 is not None:
            same = mask1 is mask0
            mask1 = mask0 if same else self._input(mask1, "mask1")
            if mask1.shape != mask0.shape:
                raise RuntimeError(f"mask1 {tuple(mask1.shape)} does not match mask0 {tuple(mask0.shape)}")
        b, h, w = mask0.shape
        widths = torch.empty((b, 2, h), dtype=torch.float32, device=mask0.device)
        area = torch.empty((b, 2), dtype=torch.int32, device=mask0.device)            # uint32 bits
        self._call("unetpp_row_widths", mask0, int(match0), mask1, int(match1), b, h, w, widths, area, stream_of=mask0)
        return widths, area.to(torch.int64) & 0xFFFFFFFF

    def width_profile(self, widths, kernel_size: int = 31, min_valid_rows: int = 20, taps=None, want_delta: bool = True):
        """The smoothing, valid rows and medians of compute_diameter_metrics (geometry_enhanced.py:144-168) for raw widths
        float32 CUDA [B,2,H] (row_widths), H <= 4096, one launch.  The kernel is geometry.gaussian_taps_f32(kernel_size)
        (an even size becomes size + 1, <= 1 means none) or `taps` (odd, at most 127 symmetric float32 values, e.g.
        cv2.getGaussianKernel's own).  Returns (smoothed float32 [B,2,H], valid uint8 [B,H], delta float32 [B,H] =
        plane 1 - plane 0 or None, dc_px float32 [B], dt_px float32 [B], valid_rows int32 [B]); the medians are 0 where
        valid_rows < min_valid_rows."""
        import torch
        from . import geometry as ge
        t = ge.resolve_taps(kernel_size, taps)
        if int(min_valid_rows) < 1:
            raise ValueError(f"min_valid_rows must be at least 1, got {min_valid_rows!r}")
        widths = self._input(widths, "widths", "[B,2,H]", "float32")
        b, _, h = widths.shape
        if h > ge.MAX_ROWS:
            raise ValueError(f"width_profile: {h} rows, at most {ge.MAX_ROWS}")
        dev = widths.device
        smoothed = torch.empty_like(widths)
        valid = torch.empty((b, h), dtype=torch.uint8, device=dev)
        delta = torch.empty((b, h), dtype=torch.float32, device=dev) if want_delta else None
        out = torch.empty((b, 3), dtype=torch.int32, device=dev)                      # {float dc_px, dt_px; int32 valid_rows}
        self._call("unetpp_width_profile", widths, b, h, t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(t), int(min_valid_rows),
                   smoothed, valid, delta, out, stream_of=widths)
        med = out[:, :2].view(torch.float32)
        return smoothed, valid, delta, med[:, 0], med[:, 1], out[:, 2]

    def components_summary(self, num, stats, min_area: int = 0):
        """The reductions analyze_defects makes of a statistics table (geometry_enhanced.py:291-294, :302-309) from `num`
        int32 [B] and `stats` int32 [B,K,5] of components() (stats may be None): int64 [B,4] on the device =
        (max(0, num - 1); labels 1..min(num, K)-1 with area >= min_area; the sum of those areas; the largest area)."""
        import torch
        num = self._input(num, "num", "[B]", "int32")
        b = num.shape[0]
        if stats is None:
            k = 2
        else:
            if not (isinstance(stats, torch.Tensor) and stats.is_cuda and stats.dtype == torch.int32 and stats.dim() == 3 and
                    stats.shape[0] == b and stats.shape[2] == 5):
                raise RuntimeError("stats must be an int32 CUDA tensor [B,K,5]")
            stats, k = stats.contiguous(), stats.shape[1]
        out = torch.empty((b, 4), dtype=torch.int64, device=num.device)
        self._call("unetpp_components_summary", num, stats, b, k, int(min_area), out, stream_of=num)
        return out

    def _filter_largest(self, pred, match_class, min_area, k):
        """filter_components(rule='largest', check=False) that also hands back `num`: (uint8 [B,H,W], int32 [B])."""
        import torch
        labels, num, stats, sums, ws, _ = self._components(pred, match_class, 8, k, True)
        b, h, w = labels.shape
        params = _lib.CcRule(float(min_area), 50.0, 300.0, 0.3, 1.6, 0.3, float(w))
        out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
        self._call("unetpp_components_filter", labels, num, stats, sums, b, h, w, k, _lib.CC_RULES["largest"], ctypes.byref(params), 1,
                   out, ws, stream_of=labels)
        return out, num

    def _profile_of_largest(self, pred, cls0, cls1, min_area, kernel_size, taps, min_valid_rows, k, want_delta):
        from . import geometry as ge
        t = ge.resolve_taps(kernel_size, taps)
        pred = self._input(pred, "pred")
        if pred.shape[1] > ge.MAX_ROWS:
            raise ValueError(f"{pred.shape[1]} rows, at most {ge.MAX_ROWS}")
        m0, n0 = self._filter_largest(pred, int(cls0), min_area, k)
        m1, n1 = self._filter_largest(pred, int(cls1), min_area, k)
        widths, area = self.row_widths(m0, -1, m1, -1)
        return self.width_profile(widths, 1, min_valid_rows, t, want_delta) + (area, (n0 > k) | (n1 > k))

    def _diameter_metrics(self, pred, cable_cls, tape_cls, mm_per_px, min_valid_rows, kernel_size, min_area, taps, k):
        import torch
        if int(min_valid_rows) < 1:
            raise ValueError(f"min_valid_rows must be at least 1, got {min_valid_rows!r}")
        _, _, _, dc, dt, rows, area, over = self._profile_of_largest(pred, cable_cls, tape_cls, min_area, kernel_size, taps,
                                                                     min_valid_rows, k, False)
        mm = float(mm_per_px)
        dc_px, dt_px = dc.to(torch.float64), dt.to(torch.float64)          # float(np.float32 median)
        dc_mm, dt_mm = dc_px * mm, dt_px * mm
        # a tensor divisor: torch divides by a Python scalar through its reciprocal, which is not the reference's quotient
        cov = area.to(torch.float64) / torch.full_like(area, pred.shape[1] * pred.shape[2], dtype=torch.float64)
        return {"dc_px": dc_px, "dt_px": dt_px, "delta_d_px": dt_px - dc_px, "dc_mm": dc_mm, "dt_mm": dt_mm,
                "delta_d_mm": dt_mm - dc_mm, "valid_rows": rows.to(torch.int64), "cable_coverage": cov[:, 0],
                "tape_coverage": cov[:, 1]}, over

    def diameter_metrics(self, pred, cable_cls: int = 1, tape_cls: int = 2, mm_per_px: float = 0.05, min_valid_rows: int = 20,
                         kernel_size: int = 31, min_area=50, taps=None, max_components: int = 8192, check: bool = True):
        """compute_diameter_metrics(pred_mask, cable_cls, tape_cls, mm_per_px, min_valid_rows)
        (src/utils/geometry_enhanced.py:113-185; kernel_size=31 and min_area=50 are the function's constants) for a uint8
        CUDA class mask [B,H,W], H <= 4096, nothing but the result leaving the device: the largest component of each
        class (filter_components, rule='largest'), one row_widths launch, one width_profile launch.  Returns a dict of
        [B] device tensors with DiameterMetrics' field names: dc_px, dt_px, delta_d_px, dc_mm, dt_mm, delta_d_mm,
        cable_coverage, tape_coverage float64 (formed as the reference forms them: float(float32 median), dt - dc,
        px * mm_per_px, dt_mm - dc_mm, area / (H W)), valid_rows int64.  Where valid_rows < min_valid_rows the six
        diameters are 0.  `taps` replaces gaussian_taps_f32(kernel_size), e.g. by cv2.getGaussianKernel's own values.
        max_components and check as for filter_components (check=True: one read-back, synchronises)."""
        k = int(max_components)
        out, over = self._diameter_metrics(pred, cable_cls, tape_cls, mm_per_px, min_valid_rows, kernel_size, min_area, taps, k)
        if check:
            self._raise_overflow(over, k, "diameter_metrics")
        return out

    def thickness_profile(self, pred, cable_cls: int = 1, tape_cls: int = 2, mm_per_px: float = 0.05, kernel_size: int = 31, taps=None):
        """compute_thickness_profile (src/utils/geometry_enhanced.py:188-225; no component filter) for a uint8 CUDA class
        mask [B,H,W], H <= 4096: {'delta_d_mm': float32 [B,H] = (tape - cable) * float32(mm_per_px), 'valid_mask': bool
        [B,H]} on the device (y_coords is arange(H)).  Two launches."""
        import torch
        from . import geometry as ge
        t = ge.resolve_taps(kernel_size, taps)
        pred = self._input(pred, "pred")
        if pred.shape[1] > ge.MAX_ROWS:
            raise ValueError(f"{pred.shape[1]} rows, at most {ge.MAX_ROWS}")
        widths, _ = self.row_widths(pred, int(cable_cls), pred, int(tape_cls))
        _, valid, delta, _, _, _ = self.width_profile(widths, 1, 1, t, True)
        mm = torch.tensor(float(np.float32(mm_per_px)), dtype=torch.float32, device=pred.device)
        return {"delta_d_mm": delta * mm, "valid_mask": valid != 0}

    def diameter_profile(self, pred, cable_cls: int, wrap_cls: int, kernel_size: int = 31, taps=None, max_components: int = 8192,
                         check: bool = True):
        """diameter_profile_from_masks(pred, cable_cls, wrap_cls) (src/utils/geometry.py:28-64, used by
        src/infer/postprocess.py:29) for a uint8 CUDA class mask [B,H,W], H <= 4096: the largest component of each class
        with no area floor, the widths per row, smooth_1d(., 31).  {'w_cable_px', 'w_wrap_px': float32 [B,H], 'valid':
        uint8 [B,H]} on the device."""
        k = int(max_components)
        sm, valid, _, _, _, _, _, over = self._profile_of_largest(pred, cable_cls, wrap_cls, 0, kernel_size, taps, 1, k, False)
        if check:
            self._raise_overflow(over, k, "diameter_profile")
        return {"w_cable_px": sm[:, 0], "w_wrap_px": sm[:, 1], "valid": valid}

    def _analyze_defects(self, pred, cable_cls, tape_cls, defect_classes, hole_min_size, k):
        import torch
        from . import morphology as mo
        pred = self._input(pred, "pred")
        defect_classes = [int(c) for c in defect_classes]
        b, h, w = pred.shape
        holes = self._morph_launch(self._morph_named("holes", (), mo.program_holes), pred, int(tape_cls), None, -1, 1)
        _, tnum, tstats, _, _, _ = self._components(pred, int(tape_cls), 8, k, True)
        tape = self.components_summary(tnum, tstats, 0)
        _, hnum, hstats, _, _, _ = self._components(holes, -1, 8, k, True)
        hole = self.components_summary(hnum, hstats, int(hole_min_size))
        _, cnum, _, _, _, _ = self._components(pred, int(cable_cls), 8, k, False)
        cable = self.components_summary(cnum, None, 0)
        _, area = self.row_widths(pred, int(tape_cls))
        tape_area = area[:, 0]
        areas = torch.zeros((b, len(defect_classes)), dtype=torch.int64, device=pred.device)
        known = [(i, c) for i, c in enumerate(defect_classes) if 0 <= c < self.num_classes]
        if known:
            counts, _ = self.mask_stats(pred)
            areas[:, [i for i, _ in known]] = counts[:, [c for _, c in known]]
        fa = tape_area.to(torch.float64)
        ratio = torch.where(tape[:, 0] > 0, tape[:, 3].to(torch.float64) / fa, torch.zeros_like(fa))
        return {"tape_hole_ratio": hole[:, 2].to(torch.float64) / tape_area.clamp(min=1).to(torch.float64),
                "tape_num_holes": hole[:, 1], "tape_coverage": fa / torch.full_like(fa, h * w), "cable_num_components": cable[:, 0],
                "tape_num_components": tape[:, 0], "tape_largest_area_ratio": ratio, "defect_areas": areas,
                "total_defect_area": areas.sum(1)}, (tnum > k) | (hnum > k)

    def analyze_defects(self, pred, cable_cls: int = 1, tape_cls: int = 2, defect_classes=(3, 4, 5, 6), hole_min_size: int = 10,
                        max_components: int = 8192, check: bool = True):
        """analyze_defects(pred_mask, cable_cls, tape_cls, defect_classes, hole_min_size)
        (src/utils/geometry_enhanced.py:246-330) for a uint8 CUDA class mask [B,H,W], every step a launch: the hole mask
        (close(tape, ELLIPSE (5,5)) - tape), the components of tape, holes and cable, components_summary of each, the
        tape area (row_widths) and the class counts (mask_stats).  Returns a dict of device tensors with DefectAnalysis'
        field names: tape_hole_ratio (hole area / max(tape area, 1)), tape_coverage, tape_largest_area_ratio (0 without
        tape) float64 [B]; tape_num_holes, cable_num_components, tape_num_components, total_defect_area int64 [B];
        defect_areas int64 [B, len(defect_classes)] in the order of defect_classes.  A defect class >= the engine's
        num_classes has area 0.  The component counts are exact whatever max_components is; the hole statistics and
        the largest tape area cover the first max_components - 1 labels: check=True (one read-back, synchronises)
        raises RuntimeError for a frame with more."""
        k = int(max_components)
        out, over = self._analyze_defects(pred, cable_cls, tape_cls, defect_classes, hole_min_size, k)
        if check:
            self._raise_overflow(over, k, "analyze_defects")
        return out

    # ------------------------------------------------------------------ stage-2 burr detection
    @staticmethod
    def _check_edge_shape(shape):
        from . import edges as ed
        h, w = int(shape[-2]), int(shape[-1])
        if h < ed.MIN_SIDE or w < ed.MIN_SIDE or h > 65535 or w > 65535 or h * w > 1 << 30:
            raise ValueError(f"image is {h}x{w}: the blur and Canny need {ed.MIN_SIDE} <= H, W <= 65535 and H * W <= 2^30")

    @staticmethod
    def _c_taps(taps):
        return None if taps is None else taps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def bgr_to_gray(self, frames):
        """cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY) for uint8 CUDA frames [B,H,W,3] -> [B,H,W] with OpenCV 4's 15-bit
        constants (unet_amd/edges.py bgr_to_gray_np)."""
        import torch
        frames = self._input(frames, "frames", "[B,H,W,3]")
        b, h, w, _ = frames.shape
        out = torch.empty((b, h, w), dtype=torch.uint8, device=frames.device)
        self._call("unetpp_gray_u8", frames, b, h, w, out, stream_of=frames)
        return out

    def gaussian_blur(self, gray, ksize: int = 5, sigma: float = 1.0, taps=None):
        """cv2.GaussianBlur(gray, (ksize, ksize), sigma) for uint8 CUDA images [B,H,W] in 8.8 fixed point with
        BORDER_REFLECT_101 (unet_amd/edges.py gaussian_blur_np); `taps` (odd, at most 7 integers summing to 256)
        replaces the kernel gaussian_taps(ksize, sigma) restates, e.g. by cv2's own.  8 <= H, W."""
        import torch
        from . import edges as ed
        t = ed.resolve_taps(ksize, sigma, taps)
        if t is None:
            raise ValueError("gaussian_blur needs a kernel: ksize >= 1 or taps")
        if hasattr(gray, "shape") and len(gray.shape) == 3:
            self._check_edge_shape(gray.shape)
        gray = self._input(gray)
        b, h, w = gray.shape
        out = torch.empty_like(gray)
        self._call("unetpp_gaussian_blur_u8", gray, b, h, w, self._c_taps(t), len(t), out, stream_of=gray)
        return out

    def canny(self, gray, low, high, blur=None):
        """cv2.Canny(gray, low, high) (aperture 3, L2gradient off) for uint8 CUDA images [B,H,W]: uint8, 0 or 255
        (unet_amd/edges.py canny_np).  blur: None, or the Gaussian blur to run first inside the same kernel, as
        (ksize, sigma) or as an integer tap array (see gaussian_blur).  The hysteresis runs on the component launches
        with a flag per root pixel: exact, the same bits from run to run, no limit on the number of fragments."""
        import torch
        from . import edges as ed
        low, high = float(low), float(high)
        if not (low >= 0 and high >= 0):
            raise ValueError(f"thresholds must be non-negative, got {low!r}, {high!r}")
        if blur is None:
            t = None
        elif isinstance(blur, tuple) and len(blur) == 2 and not isinstance(blur[0], np.ndarray):
            t = ed.resolve_taps(blur[0], blur[1], None)
        else:
            t = ed.check_taps(blur)
        if hasattr(gray, "shape") and len(gray.shape) == 3:
            self._check_edge_shape(gray.shape)
        gray = self._input(gray)
        b, h, w = gray.shape
        ws = self._workspace(("canny", b, h, w), lambda: _lib.load().unetpp_canny_workspace_bytes(b, h, w), gray.device,
                             f"canny: unsupported shape {tuple(gray.shape)}")
        out = torch.empty_like(gray)
        self._call("unetpp_canny_u8", gray, b, h, w, self._c_taps(t), 0 if t is None else len(t), low, high, out, ws, stream_of=gray)
        return out

    @staticmethod
    def _check_box(min_area, max_area, max_aspect, min_side):
        vals = [float(min_area), float(max_area), float(max_aspect), float(min_side)]
        if any(v != v for v in vals):
            raise ValueError("min_area, max_area, max_aspect and min_side must be numbers, got a NaN")
        return vals

    def filter_components_box(self, mask, match_class: int = -1, min_area=30, max_area=800, max_aspect=float("inf"), min_side=0, *,
                              connectivity: int = 8, max_components: int = 8192, out_value: int = 1, check: bool = True):
        """The component loop of detect_burrs_on_cable (infer_two_stage_burr.py:100-117) on a uint8 CUDA mask [B,H,W]:
        uint8 [B,H,W], out_value on EVERY component of (mask == match_class) with min_area <= area <= max_area,
        max(w,h) / (min(w,h) + 1e-6) < max_aspect (fp64) and w > min_side and h > min_side (unet_amd/edges.py keep_box).
        The defaults max_aspect=inf, min_side=0 leave the area clause of get_burr_mask_rulebased
        (src/refactor/burr_detector.py:53-64).  max_components and check as for filter_components."""
        box = self._check_box(min_area, max_area, max_aspect, min_side)
        out_value = self._check_out_value(out_value)
        import torch
        labels, num, stats, _, ws, _ = self._components(mask, match_class, connectivity, max_components, True)
        b, h, w = labels.shape
        k = int(max_components)
        params = _lib.CcBoxRule(*box)
        out = torch.empty((b, h, w), dtype=torch.uint8, device=labels.device)
        self._call("unetpp_components_filter_box", labels, num, stats, b, h, w, k, ctypes.byref(params), out_value, out, ws,
                   stream_of=labels)
        if check:
            self._raise_num_overflow(num, k)
        return out

    def detect_burrs(self, gray, mask_cable, match_class: int = -1, *, min_area=30, max_area=800, band_ksize: int = 8,
                     blur_ksize: int = 5, blur_sigma: float = 1.0, taps=None, canny_low=50, canny_high=150, close_ksize: int = 3,
                     open_ksize: int = 2, max_aspect=5.0, min_side=3, out_value: int = 1, max_components: int = 8192,
                     check: bool = True):
        """detect_burrs_on_cable(frame_gray, mask_cable, config) (infer_two_stage_burr.py:50-119; the defaults are the
        function's constants and its default config) for uint8 CUDA grey frames and cable masks [B,H,W], nothing leaving
        the device: canny with the blur fused -> ONE morphology launch ((dilate(cable, E8) & ~cable) & edges, close E3,
        open E2: unet_amd/edges.py program_burr) -> components -> the box rule.  Foreground of mask_cable is
        (mask == match_class), != 0 for match_class < 0.  An empty cable gives an empty band and so an empty result:
        the reference's two early returns need no read-back.  A sensitivity preset of the reference is
        detect_burrs(gray, cable, min_area=p["min_area"], max_area=p["max_area"]) with p = edges.PRESETS[name].
        uint8 [B,H,W], out_value (1 in the reference) on the kept components."""
        from . import edges as ed
        self._check_box(min_area, max_area, max_aspect, min_side)
        self._check_out_value(out_value)
        t = ed.resolve_taps(blur_ksize, blur_sigma, taps)
        ed.program_burr(band_ksize, close_ksize, open_ksize)
        self._same_shape(gray, mask_cable, "mask_cable")
        edges = self.canny(gray, canny_low, canny_high, blur=t)
        return self.burrs_from_edges(edges, mask_cable, match_class, min_area=min_area, max_area=max_area, band_ksize=band_ksize,
                                     close_ksize=close_ksize, open_ksize=open_ksize, max_aspect=max_aspect, min_side=min_side,
                                     out_value=out_value, max_components=max_components, check=check)

    def burrs_from_edges(self, edges, mask_cable, match_class: int = -1, *, min_area=30, max_area=800, band_ksize: int = 8,
                         close_ksize: int = 3, open_ksize: int = 2, max_aspect=5.0, min_side=3, out_value: int = 1,
                         max_components: int = 8192, check: bool = True):
        """detect_burrs_on_cable after its cv2.Canny call (infer_two_stage_burr.py:78-117 without :85-86) for an edge
        image `edges` (uint8 CUDA [B,H,W], non-zero = edge) from any source: one morphology launch (program_burr), the
        components, the box rule.  detect_burrs is canny() followed by this."""
        from . import edges as ed
        box = self._check_box(min_area, max_area, max_aspect, min_side)
        out_value = self._check_out_value(out_value)
        program = self._morph_named("burr", (int(band_ksize), int(close_ksize), int(open_ksize)), ed.program_burr)
        cand = self._morph_launch(program, edges, -1, mask_cable, match_class, 1)
        return self.filter_components_box(cand, 1, *box, max_components=max_components, out_value=out_value, check=check)

    def burr_mask_rulebased(self, gray, mask_cable, match_class: int = -1, *, band_out: int = 10, laplacian_threshold=30, min_area=20,
                            max_area=500, out_value: int = 255, max_components: int = 8192, check: bool = True):
        """get_burr_mask_rulebased(frame_gray, mask_cable, BurrConfig(...)) (src/refactor/burr_detector.py:11-66, defaults
        of BurrConfig) on the device: boundary_band -> |Laplacian| & 255 above the threshold inside the band (the
        reference's uint8 cast wraps above 255 and so does this) -> components -> min_area <= area <= max_area.
        uint8 [B,H,W], out_value (255 in the reference) on the kept components."""
        import math
        import torch
        from . import morphology as mo
        box = self._check_box(min_area, max_area, float("inf"), 0)
        out_value = self._check_out_value(out_value)
        thr = float(laplacian_threshold)
        if thr != thr:
            raise ValueError("laplacian_threshold must be a number")
        thr = int(math.floor(min(max(thr, -1.0), 256.0)))
        program = self._morph_named("band", (int(band_out),), mo.program_band)
        self._same_shape(gray, mask_cable, "mask_cable")
        gray = self._input(gray)
        band = self._morph_launch(program, mask_cable, match_class, None, -1, 1)
        b, h, w = gray.shape
        hot = torch.empty_like(gray)
        self._call("unetpp_laplacian_band_u8", gray, band, b, h, w, thr, hot, stream_of=gray)
        return self.filter_components_box(hot, -1, *box, max_components=max_components, out_value=out_value, check=check)

    @staticmethod
    def _same_shape(gray, other, what):
        if hasattr(gray, "shape") and hasattr(other, "shape") and tuple(gray.shape) != tuple(other.shape):
            raise RuntimeError(f"gray {tuple(gray.shape)} and {what} {tuple(other.shape)} differ in shape")

    def edges_combined(self, gray, canny_edges=None, *, blur=(5, 1.0), canny_low=30, canny_high=100, sobel_threshold=50,
                       laplacian_threshold=15):
        """edges_combined of detect_burrs_enhanced (infer_enhanced_burr.py:87-106) for uint8 CUDA grey frames [B,H,W]:
        Canny | Sobel | Laplacian, uint8 (unet_amd/edges.py edges_combined_np).  Sobel: 255 where
        uint8(sqrt(dx^2 + dy^2) / its maximum over the frame * 255) > sobel_threshold, cv2.Sobel(ksize=3) on the raw
        frame with BORDER_REFLECT_101; the per-frame maximum is reduced on the device and never read back.  A constant
        frame (0 / 0 in the reference) has no Sobel edges.  Laplacian: (|cv2.Laplacian| & 255) > laplacian_threshold.
        canny_edges: the Canny image to OR into (left unchanged), or None to run canny(gray, canny_low, canny_high,
        blur=blur) here, blur as for canny()."""
        import torch
        from . import edges as ed
        sthr, lthr = ed._u8_threshold(sobel_threshold), ed._u8_threshold(laplacian_threshold)
        if hasattr(gray, "shape") and len(gray.shape) == 3:
            self._check_edge_shape(gray.shape)
        gray = self._input(gray)
        if canny_edges is None:
            canny_edges = out = self.canny(gray, canny_low, canny_high, blur=blur)       # ORed in place: the image is ours
        else:
            self._same_shape(gray, canny_edges, "canny_edges")
            canny_edges = self._input(canny_edges, "canny_edges")
            out = torch.empty_like(gray)
        b, h, w = gray.shape
        ws = self._workspace(("edges_union", b), lambda: _lib.load().unetpp_edges_union_workspace_bytes(b), gray.device, None)
        self._call("unetpp_edges_union_u8", gray, canny_edges, b, h, w, sthr, lthr, ws, out, stream_of=gray)
        return out

    def detect_burrs_enhanced(self, gray, mask_cable, match_class: int = -1, *, min_area=50, max_area=500, band_ksize: int = 25,
                              blur_ksize: int = 5, blur_sigma: float = 1.0, taps=None, canny_low=30, canny_high=100, sobel_threshold=50,
                              laplacian_threshold=15, close_ksize: int = 5, open_ksize: int = 3, max_aspect=6.0, min_side=4,
                              out_value: int = 1, max_components: int = 8192, check: bool = True):
        """detect_burrs_enhanced(frame_gray, mask_cable, config) (infer_enhanced_burr.py:69-138; the defaults are the
        function's constants and the config 50 / 500 it is run with) for uint8 CUDA grey frames and cable masks [B,H,W],
        nothing leaving the device: edges_combined -> burrs_from_edges ((dilate(cable, E25) & ~cable) & edges, close E5,
        open E3 in one morphology launch, components, the box rule).  The reference's `width >= 5 and height >= 5` is
        the box rule's strict `> min_side` with min_side = 4.  An empty cable gives an empty band and so an empty
        result: the two early returns need no read-back.  uint8 [B,H,W], out_value (1 in the reference)."""
        from . import edges as ed
        self._check_box(min_area, max_area, max_aspect, min_side)
        self._check_out_value(out_value)
        t = ed.resolve_taps(blur_ksize, blur_sigma, taps)
        ed.program_burr(band_ksize, close_ksize, open_ksize)
        self._same_shape(gray, mask_cable, "mask_cable")
        edges = self.edges_combined(gray, blur=t, canny_low=canny_low, canny_high=canny_high, sobel_threshold=sobel_threshold,
                                    laplacian_threshold=laplacian_threshold)
        return self.burrs_from_edges(edges, mask_cable, match_class, min_area=min_area, max_area=max_area, band_ksize=band_ksize,
                                     close_ksize=close_ksize, open_ksize=open_ksize, max_aspect=max_aspect, min_side=min_side,
                                     out_value=out_value, max_components=max_components, check=check)

    def dog_band(self, gray, band, *, threshold=30, taps1=None, taps2=None):
        """255 where band != 0 and cv2.subtract(GaussianBlur(gray, 3, 1.0), GaussianBlur(gray, 7, 2.0)) > threshold, else
        0, for uint8 CUDA images [B,H,W] (src/refactor/burr_detector.py:93-103; unet_amd/edges.py dog_u8_np): both
        blurs, the saturating subtraction, the band and the threshold in one kernel.  taps1 / taps2 replace the two
        kernels (odd, at most 7 integers summing to 256, e.g. cv2's own)."""
        import torch
        from . import edges as ed
        thr = ed._u8_threshold(threshold)
        t1, t2 = ed.resolve_dog_taps(taps1, taps2)
        self._same_shape(gray, band, "band")
        if hasattr(gray, "shape") and len(gray.shape) == 3:
            self._check_edge_shape(gray.shape)
        gray, band = self._input(gray), self._input(band, "band")
        b, h, w = gray.shape
        hot = torch.empty_like(gray)
        self._call("unetpp_dog_band_u8", gray, band, b, h, w, self._c_taps(t1), len(t1), self._c_taps(t2), len(t2), thr, hot, stream_of=gray)
        return hot

    def burr_mask_dog(self, gray, mask_cable, match_class: int = -1, *, band_out: int = 10, threshold=30, min_area=20, max_area=500,
                      taps1=None, taps2=None, out_value: int = 255, max_components: int = 8192, check: bool = True):
        """get_burr_mask_dog(frame_gray, mask_cable, BurrConfig(...)) (src/refactor/burr_detector.py:69-118; `threshold`
        is the config's laplacian_threshold, which this detector reads too) on the device: boundary_band -> dog_band
        -> components -> min_area <= area <= max_area.  The subtraction of the two blurs saturates at 0, so only the
        positive lobe counts, as in the reference.  uint8 [B,H,W], out_value (255 in the reference) on the kept
        components."""
        from . import edges as ed
        from . import morphology as mo
        box = self._check_box(min_area, max_area, float("inf"), 0)
        out_value = self._check_out_value(out_value)
        ed._u8_threshold(threshold)
        ed.resolve_dog_taps(taps1, taps2)
        program = self._morph_named("band", (int(band_out),), mo.program_band)
        self._same_shape(gray, mask_cable, "mask_cable")
        if hasattr(gray, "shape") and len(gray.shape) == 3:
            self._check_edge_shape(gray.shape)
        band = self._morph_launch(program, mask_cable, match_class, None, -1, 1)
        hot = self.dog_band(gray, band, threshold=threshold, taps1=taps1, taps2=taps2)
        return self.filter_components_box(hot, -1, *box, max_components=max_components, out_value=out_value, check=check)

    def count_nonzero(self, mask):
        """np.count_nonzero per frame of a uint8 CUDA mask [B,H,W] (any H, W): int32 [B] on the device."""
        import torch
        mask = self._input(mask, "mask")
        b, h, w = mask.shape
        counts = torch.empty((b,), dtype=torch.int32, device=mask.device)      # uint32 bits; H * W <= 2^30
        self._call("unetpp_count_nonzero_u8", mask, b, h, w, counts, stream_of=mask)
        return counts

    def has_burr(self, mask, min_total_area=50):
        """has_burr(burr_mask, min_total_area) (src/refactor/burr_detector.py:121-133) for a uint8 CUDA burr mask
        [B,H,W]: bool [B] on the device, np.sum(mask > 0) >= min_total_area per frame.  Nothing is read back."""
        return self.count_nonzero(mask) >= min_total_area

    # ------------------------------------------------------------------ grey-frame enhancement (unet_amd/enhance.py is the NumPy form)
    @staticmethod
    def _c_tables(tables):
        """(unetpp_bilateral_tables, the arrays it points into) for enhance.check_tables' tuple, or (None, None)."""
        if tables is None:
            return None, None
        radius, color_w, space_w, dy, dx = tables
        f32p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
        ct = _lib.BilateralTables(radius, len(space_w), color_w.ctypes.data_as(f32p), space_w.ctypes.data_as(f32p),
                                  dy.ctypes.data_as(i32p), dx.ctypes.data_as(i32p))
        return ct, (color_w, space_w, dy, dx)

    def _enhance_input(self, frames, what="frames"):
        """uint8 CUDA [B,H,W,3] or [B,H,W], contiguous, on the engine's device -> (frames, channels)."""
        frames = self._input(frames, what, "[B,H,W,3] or [B,H,W]")
        return frames, (3 if frames.dim() == 4 else 1)

    def _enhance(self, frames, cin, cout, mode, threshold, clip_limit, tile_grid, table, tables, want_luts=False, want_decisions=False):
        """unetpp_enhance_u8: one memset and three launches on the current stream, nothing read back."""
        import torch
        from . import enhance as en
        b, h, w = frames.shape[:3]
        tx, ty = en.grid_of(tile_grid)
        en.check_limits(h, w, (tx, ty), None if tables is None else tables[0])
        if b > 65535:
            raise ValueError(f"batch {b}: at most 65535")
        dev = frames.device
        ws = self._workspace(("enhance", b, h, w, tx, ty), lambda: _lib.load().unetpp_enhance_workspace_bytes(b, h, w, tx, ty), dev,
                             f"enhance: unsupported shape {tuple(frames.shape)} with a {tx}x{ty} grid")
        out = torch.empty((b, h, w, 3) if cout == 3 else (b, h, w), dtype=torch.uint8, device=dev)
        luts = torch.empty((b, ty * tx, 256), dtype=torch.uint8, device=dev) if want_luts else None
        dec = torch.empty((b,), dtype=torch.uint8, device=dev) if want_decisions else None
        ct, keep = self._c_tables(tables)
        self._call("unetpp_enhance_u8", frames, b, h, w, cin, cout, mode, float(threshold), float(clip_limit), tx, ty,
                   None if table is None else table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                   None if ct is None else ctypes.byref(ct), out, luts, dec, ws, stream_of=frames)
        del keep
        return out, luts, dec

    def is_grayscale(self, frames, threshold: float = 10.0, return_sums: bool = False):
        """is_grayscale_frame (src/refactor/preprocess.py:12-32) for uint8 CUDA frames [B,H,W,3]: bool [B] on the device,
        max(sum |b - g|, sum |g - r|, sum |r - b|) / (H W) < threshold as one float64 division of exact integers
        (enhance.is_grayscale_np).  Frames [B,H,W] count as grey.  return_sums: also the three sums, int64 [B,3]."""
        import torch
        frames, cin = self._enhance_input(frames)
        b, h, w = frames.shape[:3]
        if cin == 1:
            dec = torch.ones((b,), dtype=torch.bool, device=frames.device)
            return (dec, torch.zeros((b, 3), dtype=torch.int64, device=frames.device)) if return_sums else dec
        dec = torch.empty((b,), dtype=torch.uint8, device=frames.device)
        sums = torch.empty((b, 3), dtype=torch.int64, device=frames.device)      # uint64 bits, far below 2^63
        self._call("unetpp_gray_decision", frames, b, h, w, float(threshold), dec, sums, stream_of=frames)
        return (dec != 0, sums) if return_sums else dec != 0

    def clahe(self, gray, clip_limit: float = 2.0, tile_grid=(8, 8), return_luts: bool = False):
        """cv2.createCLAHE(clip_limit, tile_grid).apply(gray) for uint8 CUDA images [B,H,W] as OpenCV's CLAHE_Impl::apply
        computes it (enhance.clahe_np; cv2's own result is unpinned).  tile_grid = (tilesX, tilesY) or one number, 1..16
        per side, H > tilesY, W > tilesX.  return_luts: also the per-tile tables uint8 [B, tilesY * tilesX, 256]."""
        gray = self._input(gray)
        out, luts, _ = self._enhance(gray, 1, 1, _lib.ENHANCE_ALWAYS, 0.0, clip_limit, tile_grid, None, None, want_luts=return_luts)
        return (out, luts) if return_luts else out

    def bilateral_filter(self, gray, d: int = 5, sigma_color: float = 75.0, sigma_space: float = 75.0, tables=None):
        """cv2.bilateralFilter(gray, d, sigma_color, sigma_space) for uint8 CUDA images [B,H,W] as OpenCV's scalar 8-bit
        loop computes it (enhance.bilateral_np; cv2's own result is unpinned), radius <= 4 (d <= 9), H, W > radius.
        tables: enhance.bilateral_tables' tuple instead, e.g. with cv2's own weights or tap order."""
        import torch
        from . import enhance as en
        tables = en.check_tables(en.bilateral_tables(d, sigma_color, sigma_space) if tables is None else tables)
        gray = self._input(gray)
        b, h, w = gray.shape
        en.check_limits(h, w, None, tables[0])
        out = torch.empty_like(gray)
        ct, keep = self._c_tables(tables)
        self._call("unetpp_bilateral_u8", gray, b, h, w, ctypes.byref(ct), out, stream_of=gray)
        del keep
        return out

    def enhance_grayscale(self, frames, *, clip_limit: float = 2.0, tile_grid=8, gamma: float = 0.8, denoise_method: str = "bilateral",
                          denoise_strength: int = 5, channels_out: int = 3):
        """enhance_grayscale_frame (src/refactor/preprocess.py:35-74) for uint8 CUDA frames [B,H,W,3] (BGR) or [B,H,W]:
        BGR2GRAY, CLAHE, the gamma table, cv2.bilateralFilter(denoise_strength, 75, 75), GRAY2BGR -> uint8 [B,H,W,3]
        (channels_out = 1: [B,H,W]); every frame is enhanced.  Defaults are PreprocessConfig's.  One memset and three
        launches, nothing read back (enhance.enhance_grayscale_np is the NumPy form).  denoise_method other than
        'bilateral' filters nothing, as in the reference; 'fastNlMeans' is a ValueError."""
        from . import enhance as en
        if channels_out not in (1, 3):
            raise ValueError(f"channels_out must be 1 or 3, got {channels_out!r}")
        tables = en.denoise_tables(denoise_method, denoise_strength)
        tables = None if tables is None else en.check_tables(tables)
        frames, cin = self._enhance_input(frames)
        return self._enhance(frames, cin, int(channels_out), _lib.ENHANCE_ALWAYS, 0.0, clip_limit, tile_grid, en.gamma_table(gamma), tables)[0]

    def preprocess_frames(self, frames, enable: bool = True, threshold: float = 10.0, *, clip_limit: float = 2.0, tile_grid=8,
                          gamma: float = 0.8, denoise_method: str = "bilateral", denoise_strength: int = 5, return_decisions: bool = False):
        """preprocess_frame (src/refactor/preprocess.py:77-91) for a batch of uint8 CUDA frames [B,H,W,3]: the frames
        is_grayscale_frame calls grey are enhanced (enhance_grayscale), the others copied, decided per frame ON THE DEVICE
        -- no synchronisation and no read-back between the first and the last launch.  enable=False
        (PreprocessConfig.enable_grayscale_enhance) copies every frame.  Frames [B,H,W] always count as grey and come
        back as [B,H,W,3].  return_decisions: also bool [B], True where a frame was enhanced."""
        import torch
        from . import enhance as en
        tables = en.denoise_tables(denoise_method, denoise_strength)
        tables = None if tables is None else en.check_tables(tables)
        frames, cin = self._enhance_input(frames)
        if not enable:
            out = frames.clone() if cin == 3 else frames[..., None].expand(-1, -1, -1, 3).contiguous()
            return (out, torch.zeros((frames.shape[0],), dtype=torch.bool, device=frames.device)) if return_decisions else out
        out, _, dec = self._enhance(frames, cin, 3, _lib.ENHANCE_IF_GREY, threshold, clip_limit, tile_grid, en.gamma_table(gamma), tables,
                                    want_decisions=return_decisions)
        return (out, dec != 0) if return_decisions else out

    def resize_frames(self, frames, size_hw):
        """cv2.resize(frame, (W, H), interpolation=cv2.INTER_LINEAR) for uint8 CUDA frames [B,h,w,C] -> [B,H,W,C]
        (preprocess_image, infer_two_stage_burr.py:124).  Chain with segment(): the BGR->RGB swap and /255 run
        inside the engine's first kernel."""
        import torch
        frames = self._input(frames, "frames", "[B,H,W,C]")
        H, W = int(size_hw[0]), int(size_hw[1])
        b, h, w, c = frames.shape
        out = torch.empty((b, H, W, c), dtype=torch.uint8, device=frames.device)
        self._call("unetpp_resize_linear_u8", frames, b, h, w, c, out, H, W, stream_of=frames, invalid=RuntimeError)
        return out

    def resize_masks(self, pred, frame_size_wh, match_class: int = -1, roi=None):
        """infer_two_stage_burr.py:303-314 on the device for a uint8 CUDA mask [B,H,W]: optional
        `(pred == match_class)`, cv2.resize(..., (width, height), INTER_NEAREST), zeros outside
        roi = (x1, y1, x2, y2).  Returns uint8 [B,height,width]."""
        import torch
        pred = self._input(pred, "pred")
        fw, fh = int(frame_size_wh[0]), int(frame_size_wh[1])
        x1, y1, x2, y2 = (0, 0, fw, fh) if roi is None else (int(v) for v in roi)
        b, h, w = pred.shape
        out = torch.empty((b, fh, fw), dtype=torch.uint8, device=pred.device)
        self._call("unetpp_resize_nearest_roi_u8", pred, b, h, w, int(match_class), out, fh, fw, x1, y1, x2, y2, stream_of=pred,
                   invalid=RuntimeError)
        return out

    # ------------------------------------------------------------------ sliding-window inference (unet_amd/tiling.py is the NumPy form)
    @staticmethod
    def _c_origins(plan):
        ys, xs = np.asarray(plan.ys, np.int32), np.asarray(plan.xs, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        return ys, xs, ys.ctypes.data_as(i32p), xs.ctypes.data_as(i32p)

    @staticmethod
    def _check_plan(plan, h, w, patch_size):
        from . import tiling as tl
        if plan.n_patches == 0:
            raise ValueError(f"the plan for {h}x{w} at patch_size {patch_size} has no patch")
        if len(plan.ys) > tl.MAX_AXIS or len(plan.xs) > tl.MAX_AXIS:
            raise ValueError(f"unsupported: a plan of {len(plan.ys)}x{len(plan.xs)} patches, at most {tl.MAX_AXIS} per axis")

    def _check_target_size(self, target_size):
        t = int(target_size)
        if t < self._SIZE_MULTIPLE or t % self._SIZE_MULTIPLE:
            raise ValueError(f"target_size must be a positive multiple of {self._SIZE_MULTIPLE}, got {target_size!r}")
        return t

    def gather_tiles(self, frames, patch_size: int = 384, stride: int = 192, target_size: int = 256, channel_order: str = "rgb"):
        """The patch batch of SlidingWindowInference.predict (tools/inference_binary_patch.py:56-82) for uint8 CUDA frames
        [B,H,W,3], in one launch: crop at tiling.tile_plan's origins, reflect padding at the bottom and right, cv2's uint8
        INTER_LINEAR resize to target_size.  Returns uint8 [B * P, T, T, 3] (frame-major, plan order inside a frame) in
        BGR, what forward / segment / predict_proba take: channel_order="rgb" (the reference's predict gets RGB frames)
        reverses the channels, "bgr" keeps them."""
        import torch
        from . import tiling as tl
        if channel_order not in tl.CHANNEL_ORDERS:
            raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
        t = self._check_target_size(target_size)
        frames = self._input(frames, "frames", "[B,H,W,3]")
        b, h, w, _ = frames.shape
        plan = tl.tile_plan(h, w, patch_size, stride)
        self._check_plan(plan, h, w, patch_size)
        tl.check_padding(h, w, int(patch_size))
        ys, xs, pys, pxs = self._c_origins(plan)
        out = torch.empty((b * plan.n_patches, t, t, 3), dtype=torch.uint8, device=frames.device)
        self._call("unetpp_tile_gather_u8", frames, b, h, w, pys, len(ys), pxs, len(xs), int(patch_size), t, tl.CHANNEL_ORDERS[channel_order],
                   out, stream_of=frames)
        return out

    def tile_gate(self, maps, gate_thr, gate_class: int = 1):
        """The window gate of OptimizedSlidingWindowInference.predict (tools/inference_binary_optimized.py:91-98) for
        probability maps float32 CUDA [N,C,T,T]: (include uint8 [N] = score >= gate_thr, scores float32 [N] = the maximum
        of class gate_class over the patch), one launch, nothing read back."""
        import torch
        maps = self._input(maps, "maps", "[N,C,T,T]", "float32")
        n, c, t, _ = maps.shape
        if not 0 <= int(gate_class) < c:
            raise ValueError(f"gate_class {gate_class} not in [0,{c})")
        scores = torch.empty((n,), dtype=torch.float32, device=maps.device)
        include = torch.empty((n,), dtype=torch.uint8, device=maps.device)
        self._call("unetpp_tile_gate_f32", maps, n, c, t, int(gate_class), float(gate_thr), scores, include, stream_of=maps)
        return include, scores

    def blend_tiles(self, maps, frame_hw, patch_size: int = 384, stride: int = 192, include=None, return_output: bool = True):
        """The fold of predict (tools/inference_binary_patch.py:98-113) for per-patch maps float32 CUDA [B * P, C, T, T] of
        B frames of frame_hw = (H, W), in one launch: each map resized to patch_size (float32 INTER_LINEAR), cropped, summed
        in plan order, divided by count + 1e-8, argmax.  `include` uint8 CUDA [B * P] (tile_gate) drops patches.  Returns
        (mask uint8 [B,H,W], output float32 [B,H,W,C] or None)."""
        import torch
        from . import tiling as tl
        h, w = int(frame_hw[0]), int(frame_hw[1])
        plan = tl.tile_plan(h, w, patch_size, stride)
        self._check_plan(plan, h, w, patch_size)
        maps = self._input(maps, "maps", "[N,C,T,T]", "float32")
        n, c, t, _ = maps.shape
        if n % plan.n_patches:
            raise RuntimeError(f"maps hold {n} patches, the plan for {h}x{w} has {plan.n_patches} per frame")
        if c > tl.MAX_CLASSES:
            raise ValueError(f"unsupported: {c} classes, at most {tl.MAX_CLASSES}")
        b = n // plan.n_patches
        if include is not None:
            include = self._input(include, "include", f"[{n}]")
        ys, xs, pys, pxs = self._c_origins(plan)
        mask = torch.empty((b, h, w), dtype=torch.uint8, device=maps.device)
        output = torch.empty((b, h, w, c), dtype=torch.float32, device=maps.device) if return_output else None
        self._call("unetpp_tile_blend_f32", maps, b, c, t, pys, len(ys), pxs, len(xs), int(patch_size), include, h, w, mask, output,
                   stream_of=maps)
        return mask, output

    def predict_tiled(self, frames, patch_size: int = 384, stride: int = 192, target_size: int = 256, blend: str = "logits",
                      gate_thr=None, gate_class: int = 1, channel_order: str = "rgb", return_output: bool = True):
        """SlidingWindowInference.predict (tools/inference_binary_patch.py:36-115; blend="logits") or
        OptimizedSlidingWindowInference.predict (tools/inference_binary_optimized.py:40-113; blend="probs", softmax maps,
        gate_thr=None is use_gating=False) for uint8 CUDA frames [B,H,W,3] of any size, without leaving the device:
        gather_tiles, the network on the patches of all frames in chunks of at most max_batch, tile_gate, blend_tiles.
        Returns (mask uint8 [B,H,W], output float32 [B,H,W,C] or None); a plan with no patch gives zeros, as the
        reference does."""
        import torch
        from . import tiling as tl
        if blend not in tl.BLENDS:
            raise ValueError(f"blend must be 'logits' or 'probs', got {blend!r}")
        if gate_thr is not None and blend != "probs":
            raise ValueError("gate_thr needs blend='probs': the gate score is a probability")
        if channel_order not in tl.CHANNEL_ORDERS:
            raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
        t = self._check_target_size(target_size)
        frames = self._input(frames, "frames", "[B,H,W,3]")
        b, h, w, _ = frames.shape
        c, dev = self.num_classes, frames.device
        plan = tl.tile_plan(h, w, patch_size, stride)
        if plan.n_patches == 0:
            return (torch.zeros((b, h, w), dtype=torch.uint8, device=dev),
                    torch.zeros((b, h, w, c), dtype=torch.float32, device=dev) if return_output else None)
        patches = self.gather_tiles(frames, patch_size, stride, t, channel_order)
        n = patches.shape[0]
        maps = torch.empty((n, c, t, t), dtype=torch.float32, device=dev)
        step = max(1, self._max_batch)
        for k in range(0, n, step):                 # the engine writes each chunk's maps into its slice: no copy
            x, fmt, nb, _, _ = self._prepare(patches[k:k + step])
            dst = maps[k:k + nb].data_ptr()
            outs = _lib.Outputs(dst if blend == "logits" else None, dst if blend == "probs" else None, None, None, None,
                                _lib.RULES["argmax"], 0.0, 0.0, 0.0, 0.0)
            self._call("unetpp_forward_ex", x, fmt, nb, t, t, ctypes.byref(outs), stream_of=x, invalid=RuntimeError)
        if self._check_range:
            self.raise_on_range_error()
        include = None if gate_thr is None else self.tile_gate(maps, gate_thr, gate_class)[0]
        return self.blend_tiles(maps, (h, w), patch_size, stride, include, return_output)
